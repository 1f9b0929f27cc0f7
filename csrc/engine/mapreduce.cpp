// Native MapReduce object (see mapreduce.h). Reference behaviour cited per
// method as src/mapreduce.cpp:<lines>.
#include "devfn.h"
#include "hostarena.h"
#include "xfer.h"
#include "mapreduce.h"
#include "guard.h"
#include "hbmpool.h"
#include "grouper.h"
#include "guardalloc.h"
#include "ooc.h"

#include <c10/hip/HIPCachingAllocator.h>
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <filesystem>
#include <fstream>
#include <numeric>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string_view>

namespace mrh {

std::atomic<int> MapReduce::instances_now{0}, MapReduce::instances_ever{0};
std::atomic<int64_t> MapReduce::msize{0}, MapReduce::msizemax{0}, MapReduce::rsize{0}, MapReduce::wsize{0},
    MapReduce::cssize{0}, MapReduce::crsize{0};
double MapReduce::commtime = 0.0;

std::function<void(const std::string&)>& screen_sink() {
  static std::function<void(const std::string&)> f = [](const std::string& s) {
    std::fwrite(s.data(), 1, s.size(), stdout);
    std::fflush(stdout);
  };
  return f;
}

namespace {

thread_local int g_op_depth = 0;
void device_sync(const MapReduce* mr) {
  if (mr->device().is_cuda()) guard::hip_check(hipDeviceSynchronize(), "trace_sync", mr->comm()->rank());
}

[[noreturn]] void fail(const std::string& m) { throw std::runtime_error(m); }

void out(const std::string& s) { screen_sink()(s); }

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}

// one column (keys or values) staged to host memory
struct HostCol {
  at::Tensor data, off;
  int w = 0;
  int64_t base = 0;             // byte shift that makes data + base aligned (aligned layouts)
  std::vector<int64_t> pstart;  // padded row starts (keyalign / valuealign layouts), else empty
  char* d() const { return data.numel() ? (char*)data.data_ptr<uint8_t>() + base : nullptr; }
  int64_t a(int64_t i) const {
    if (!pstart.empty()) return pstart[i];
    return w >= 0 ? i * w : off.data_ptr<int64_t>()[i];
  }
  int64_t len(int64_t i) const { return w >= 0 ? w : off.data_ptr<int64_t>()[i + 1] - off.data_ptr<int64_t>()[i]; }
  char* at(int64_t i) const { return d() ? d() + a(i) : nullptr; }
};
HostCol host_col(const at::Tensor& data, const at::Tensor& off, int w) {
  HostCol c;
  c.data = data.defined() ? data.to(at::kCPU).contiguous() : at::empty({0}, at::TensorOptions().dtype(at::kByte));
  c.off = (w < 0) ? off.to(at::kCPU).contiguous() : at::Tensor();
  c.w = w;
  return c;
}

// keyalign / valuealign (reference src/keyvalue.cpp:345-352, page layout
// `kb | vb | pad | key | pad | value`): the pointer a host callback receives
// for each key (or KV value) is a multiple of `align`; for KMV multivalues
// (seg given) the start of each key's value list is aligned and its values
// stay packed back to back, as in the reference KMV page (src/keymultivalue.
// cpp:830-839). Alignments must be powers of two (src/mapreduce.cpp:3327-3332).
void align_col(HostCol& c, int64_t n, int align, const int64_t* seg = nullptr, int64_t nseg = 0, bool zero = false) {
  if (align < 1 || (align & (align - 1))) throw std::runtime_error("Invalid alignment (keyalign/valuealign must be a power of 2)");
  if (align == 1 || n == 0) return;
  auto up = [&](int64_t x) { return (x + align - 1) & ~(int64_t)(align - 1); };
  std::vector<int64_t> st((size_t)n);
  int64_t pos = 0;
  bool same = ((uintptr_t)c.d() % align) == 0;
  auto place = [&](int64_t i, bool aligned_start) {
    if (aligned_start) pos = up(pos);
    st[i] = pos;
    same = same && pos == c.a(i);
    pos += c.len(i);
  };
  if (seg) {
    for (int64_t s = 0; s < nseg; ++s)
      for (int64_t i = seg[s]; i < seg[s + 1]; ++i) place(i, i == seg[s]);
  } else {
    for (int64_t i = 0; i < n; ++i) place(i, true);
  }
  if (same) return;  // already aligned in place (e.g. fixed widths that are multiples of align)
  // zeropage (reference: pages zeroed when allocated): padding bytes are 0
  at::Tensor buf = zero ? at::zeros({pos + align}, at::TensorOptions().dtype(at::kByte))
                        : at::empty({pos + align}, at::TensorOptions().dtype(at::kByte));
  const int64_t shift = (align - (int64_t)((uintptr_t)buf.data_ptr<uint8_t>() % align)) % align;
  char* dst = (char*)buf.data_ptr<uint8_t>() + shift;
  for (int64_t i = 0; i < n; ++i)
    if (c.len(i)) std::memcpy(dst + st[i], c.at(i), (size_t)c.len(i));
  c.data = buf;
  c.base = shift;
  c.pstart = std::move(st);
}

KV clone_kv(const KV& kv) {
  KV o = kv;
  o.kdata = kv.kdata.clone();
  o.vdata = kv.vdata.clone();
  if (kv.koff.defined()) o.koff = kv.koff.clone();
  if (kv.voff.defined()) o.voff = kv.voff.clone();
  return o;
}
KMV clone_kmv(const KMV& m) {
  KMV o = m;
  o.keys = clone_kv(m.keys);
  o.vdata = m.vdata.clone();
  if (m.voff.defined()) o.voff = m.voff.clone();
  o.seg = m.seg.clone();
  return o;
}
at::Tensor to_host(const at::Tensor& t, bool pin) {
  if (!t.defined()) return t;
  note_xfer(t, at::Device(at::kCPU));
  if (pin && t.is_cuda()) {  // one copy, straight into pinned memory (not pageable, then pinned)
    at::Tensor h = hostarena::pinned_empty(t.sizes(), t.scalar_type());
    h.copy_(t);
    return h;
  }
  return t.to(at::kCPU);
}
KV kv_host(const KV& kv, bool pin) {
  KV o = kv;
  o.kdata = to_host(kv.kdata, pin);
  o.vdata = to_host(kv.vdata, pin);
  o.koff = to_host(kv.koff, pin);
  o.voff = to_host(kv.voff, pin);
  return o;
}
KMV kmv_to(const KMV& m, at::Device d, bool pin) {
  KMV o = m;
  if (d.is_cpu()) {
    o.keys = kv_host(m.keys, pin);
    o.vdata = to_host(m.vdata, pin);
    o.voff = to_host(m.voff, pin);
    o.seg = to_host(m.seg, pin);
  } else {
    o.keys = kv_to(m.keys, d);
    for (const at::Tensor* t : {&m.vdata, &m.voff, &m.seg}) note_xfer(*t, d);
    o.vdata = m.vdata.to(d);
    if (m.voff.defined()) o.voff = m.voff.to(d);
    o.seg = m.seg.to(d);
  }
  return o;
}

std::string fmt_item(const char* p, int64_t n, int flag) {
  switch (flag) {
    case 0: return "NULL";
    case 1: { int32_t x = 0; std::memcpy(&x, p, std::min<int64_t>(n, 4)); return std::to_string(x); }
    case 2: { uint64_t x = 0; std::memcpy(&x, p, std::min<int64_t>(n, 8)); return std::to_string(x); }
    case 3: { float x = 0; std::memcpy(&x, p, std::min<int64_t>(n, 4)); return fmt("%g", x); }
    case 4: { double x = 0; std::memcpy(&x, p, std::min<int64_t>(n, 8)); return fmt("%g", x); }
    case 5: return std::string(p, strnlen(p, (size_t)n));
    case 6: { int32_t x[2] = {0, 0}; std::memcpy(x, p, std::min<int64_t>(n, 8)); return fmt("%d %d", x[0], x[1]); }
    case 7: { uint64_t x[2] = {0, 0}; std::memcpy(x, p, std::min<int64_t>(n, 16));
              return fmt("%" PRIu64 " %" PRIu64, x[0], x[1]); }
  }
  fail("Invalid print args");
}

void expand_path(const std::string& path, int recurse, std::vector<std::string>& outv) {
  namespace fs = std::filesystem;
  std::error_code ec;
  if (fs::is_regular_file(path, ec)) {
    outv.push_back(path);
  } else if (fs::is_directory(path, ec)) {
    std::vector<std::string> names;
    for (auto& e : fs::directory_iterator(path)) names.push_back(e.path().filename().string());
    std::sort(names.begin(), names.end());
    for (auto& n : names) {
      std::string full = (fs::path(path) / n).string();
      if (fs::is_regular_file(full, ec)) outv.push_back(full);
      else if (recurse && fs::is_directory(full, ec)) expand_path(full, recurse, outv);
    }
  } else {
    fail("Invalid filename " + path);
  }
}

std::string join(const std::vector<std::string>& v) {
  std::string s;
  for (auto& x : v) {
    s += x;
    s.push_back('\n');
  }
  return s;
}
std::vector<std::string> split_lines(const std::string& s) {
  std::vector<std::string> v;
  size_t a = 0;
  while (a < s.size()) {
    size_t b = s.find('\n', a);
    if (b == std::string::npos) b = s.size();
    v.push_back(s.substr(a, b - a));
    a = b + 1;
  }
  return v;
}

struct ChunkTask {
  int ifile, itask, ntask;
  int64_t fsize;
};

}  // namespace

// ====================================================================== op frame

// The frame every op runs in: a stack object constructed at the top of the
// op, the only thing an op needs for protocol. It holds the op's start state
// (wall clock and comm counters, read once: the stats lines and the MRH_TRACE
// record both measure from them), so an op that runs other ops (collate,
// scrunch) keeps its own.
//
// Construction opens a roctx range (`rocprofv3 --marker-trace` shows every op
// around its kernels and RCCL calls) and, with MRH_TRACE set, the op's trace
// record (guard.h trace_op: wall time with the device synchronised at both
// ends, local pair counts and bytes, the bytes this rank sent / received in
// shuffles), then runs the entry protocol (enter). The finishers print the
// stats and return the global count. On scope exit, after the return value
// is computed, an MR with outofcore == 1 writes its data to disk — the
// reference's forced out-of-core mode (src/keyvalue.cpp:122,223); the next op
// reads it back.
class MapReduce::Op {
 public:
  struct Deferred {};
  // the map family drops the data it replaces (drop_for_map) after the trace
  // opens and before the entry protocol: it calls enter() itself
  Op(MapReduce* mr, const char* name, Deferred) : mr_(mr), name_(name) {
    if (mr->set.timer == 1) mr->comm_->barrier();
    mark();
    roctxRangePushA(name);
    if (g_op_depth == 0) guard::set_current_op(name);
    // page pool installed + a page budget B: the op may hold at most 2B of
    // new device memory (output + working set) plus 16 MiB of kernel scratch
    // (sort histograms, scan partials, size-class rounding); past it an
    // allocation fails with "Cannot allocate page" (reference mem_request at
    // maxpage)
    if (g_op_depth == 0 && hbm::installed() && mr->device().is_cuda() && mr->budget() > 0)
      cap_.emplace(mr->device().index() < 0 ? 0 : mr->device().index(), 2 * mr->budget() + (int64_t(16) << 20));
    if (guard::trace_enabled()) device_sync(mr);
    ++g_op_depth;
  }
  // parts_ok: the op reads the appended KV parts itself (else they are
  // flattened); kmv_parts_ok: the same for the KMV's parts
  Op(MapReduce* mr, const char* name, bool ooc_ok = false, bool parts_ok = false, bool kmv_parts_ok = false)
      : Op(mr, name, Deferred()) {
    enter(ooc_ok, parts_ok, kmv_parts_ok);
  }
  // close(): the end of an open() .. close() span, not an op of its own (no
  // trace record, no entry protocol); its stats measure from here
  explicit Op(MapReduce* mr) : mr_(mr), name_(nullptr) { mark(); }
  Op(const Op&) = delete;
  Op& operator=(const Op&) = delete;

  ~Op() {
    if (!name_) return;
    --g_op_depth;
    if (std::uncaught_exceptions() > 0 && g_op_depth == 0 && mr_->comm()->size() > 1) {
      // an op failing on one rank can never complete its collectives on the
      // others: fail the whole job now (reference Error::one -> MPI_Abort,
      // src/error.cpp:47-57) instead of leaving peers blocked in a shuffle
      mr_->comm()->poison(std::string("MapReduce ") + name_ + " raised an error on rank " +
                          std::to_string(mr_->my_proc()));
    }
    if (guard::trace_enabled() && std::uncaught_exceptions() == 0) {
      device_sync(mr_);
      const double t1 = Comm::wtime();
      int64_t b = 0;
      if (mr_->kv) b += mr_->kv->nbytes();
      for (const KMV& m : mr_->kmv_parts()) b += m.nbytes();
      guard::trace_op(mr_->my_proc(), name_, mr_->instance(), g_op_depth, began_, (t1 - began_) * 1e3,
                      mr_->kv ? mr_->kv->n : 0, mr_->kmv_keys(), b, cssize.load() - sent0_, crsize.load() - recv0_);
    }
    // freepage (reference: pages freed after every op, src/mapreduce.cpp:
    // 3483-3517): with an HBM budget in force, blocks the op freed go back to
    // the driver too, so the footprint between ops stays within the budget
    if (mr_->set.freepage && mr_->budget() > 0 && g_op_depth == 0 && mr_->device().is_cuda() &&
        std::uncaught_exceptions() == 0)
      c10::hip::HIPCachingAllocator::emptyCache();
    // MRH_GUARD: every live block's canaries at the end of each top-level op
    if (g_op_depth == 0 && guard::alloc_guard_active()) {
      guard::check_all_blocks(name_);
      guard::set_current_op(nullptr);
    }
    if (mr_->set.outofcore == 1 && std::uncaught_exceptions() == 0) {
      try {
        mr_->spill_disk();
      } catch (const std::exception& e) {
        std::fprintf(stderr, "mrhip: out-of-core write failed: %s\n", e.what());
      }
    }
    roctxRangePop();
  }

  // every op's entry: fault injection point, and data spilled to host (spill()
  // or spill-on-OOM) comes back to HBM before the op touches it
  void enter(bool ooc_ok = false, bool parts_ok = false, bool kmv_parts_ok = false) {
    MapReduce& m = *mr_;
    guard::fault_point(name_, m.comm_->rank());
    if (!parts_ok) m.flatten();
    if (!kmv_parts_ok) m.flatten_kmv();
    if (guard::alloc_guard_active()) {  // an overrun found at the end of an earlier op fails the next one
      static size_t raised = 0;
      const auto reps = guard::guard_reports();
      if (reps.size() > raised) {
        const guard::GuardReport& r = reps[raised];
        raised = reps.size();
        throw std::runtime_error("mrhip guard: out-of-bounds device write into a " + std::to_string(r.size) +
                                 "-byte block allocated in " + r.alloc_op + ", detected " + r.found_op);
      }
    }
    if (!m.started_) {
      m.started_ = true;
      // minpage (reference allocate(), src/mapreduce.cpp:3318-3357): pages
      // claimed up front; here the caching allocator's pool is grown by
      // minpage x memsize once, so the first ops do not pay for hipMalloc
      if (m.set.minpage > 0 && m.device().is_cuda()) {
        at::Tensor t = at::empty({(int64_t)m.set.minpage * m.block_bytes()},
                                 at::TensorOptions().device(m.device()).dtype(at::kByte));
      }
    }
    m.ensure_resident();
    // a group-by index outlives its KV only until the next op sees the KV changed
    if (m.grouped_ && (!m.kv || !m.grouped_->describes(*m.kv))) m.grouped_.reset();
    const bool on_host = (m.kv && !m.kv->device().is_cuda()) || (m.kmv && !m.kmv->keys.device().is_cuda());
    if (!m.device().is_cuda() || !on_host) return;
    // an op with an out-of-core path leaves host-resident data larger than the
    // HBM budget where it is and streams it; every other op brings it back
    if (ooc_ok && needs_ooc(m.data_bytes(), m.budget(), 2.0)) return;
    m.unspill();
  }

  // The finishers: the op's stats lines, then the global count it returns.
  // These are the pairs of the KV / the keys of the KMV with their appended
  // parts. Where an op used to count kv->n or kmv->nkey alone it had entered
  // with parts_ok / kmv_parts_ok false, so the parts were flattened at entry
  // and its body assigns kv / kmv whole: the tail is empty and the two agree.
  uint64_t kv_done(const char* heading) {
    stats(heading, 0);
    return mr_->count(mr_->kv_rows());
  }
  uint64_t kmv_done(const char* heading) {
    stats(heading, 1);
    return mr_->count(mr_->kmv_keys());
  }

 private:
  void mark() {
    began_ = Comm::wtime();
    sent0_ = cssize.load();
    recv0_ = crsize.load();
  }

  // per-op stats (reference :3112-3179)
  void stats(const char* heading, int which) {
    MapReduce& m = *mr_;
    Comm& comm = *m.comm_;
    if (guard::check_enabled()) {
      if (m.kv) guard::check_kv(*m.kv, heading);
      for (const KMV& p : m.kmv_parts()) guard::check_kmv(p, heading);
    }
    const int64_t b = m.data_bytes();
    msize = b;
    if (b > msizemax) msizemax = b;
    if (m.set.timer == 1) {
      comm.barrier();
      if (comm.rank() == 0) out(fmt("%s time (secs) = %g\n", heading, Comm::wtime() - began_));
    } else if (m.set.timer == 2) {
      m.histo(Comm::wtime() - began_, (std::string(heading) + " time (secs) =").c_str());
    }
    if (m.set.verbosity == 0) return;
    if (comm.rank() == 0) out(std::string(heading) + (which == 0 ? " KV = " : " KMV = "));
    if (which == 0) m.kv_stats(m.set.verbosity);
    else m.kmv_stats(m.set.verbosity);
    std::vector<int64_t> sr = comm.allreduce({cssize - sent0_, crsize - recv0_}, Comm::SUM);
    if (sr[0] || sr[1]) {
      const double mb = 1024.0 * 1024.0;
      if (comm.rank() == 0) out(fmt("%s Comm = %.3g Mb send, %.3g Mb recv\n", heading, sr[0] / mb, sr[1] / mb));
      if (m.set.verbosity == 2) {
        m.histo((cssize - sent0_) / mb, "  Send (Mb):");
        m.histo((crsize - recv0_) / mb, "  Recv (Mb):");
      }
    }
  }

  MapReduce* mr_;
  const char* name_;
  double began_ = 0;
  int64_t sent0_ = 0, recv0_ = 0;
  std::optional<hbm::OpCap> cap_;
};

namespace {
// collate and scrunch run their inner ops silently: the caller's verbosity and
// timer come back on scope exit, also when an inner op throws
struct Quiet {
  explicit Quiet(Settings& s) : set_(s), verbosity_(s.verbosity), timer_(s.timer) { s.verbosity = s.timer = 0; }
  ~Quiet() {
    set_.verbosity = verbosity_;
    set_.timer = timer_;
  }
  Settings& set_;
  const int verbosity_, timer_;
};
}  // namespace

// ====================================================================== lifecycle

MapReduce::MapReduce(CommPtr comm) : comm_(std::move(comm)) {
  if (!comm_) comm_ = std::make_shared<Comm>();
  if (const char* p = std::getenv("MRMPI_FPATH")) set.fpath = p;
  instances_now++;
  instance_me_ = ++instances_ever;
  guard::register_mr(this);
}

MapReduce::~MapReduce() {
  drop_disk();
  guard::unregister_mr(this);
  instances_now--;
}

// A map/reduce builder of an MR with an HBM or host budget is bounded: its
// chunks go through a Spool (HBM share of the budget, then pinned host up to
// host_budget, then files under fpath), pieces of memsize bytes at most
void MapReduce::bound(KeyValue& b) {
  if (budget() <= 0 && set.host_budget <= 0) return;
  SpoolConfig c;
  c.budget->hbm = budget() > 0 && device().is_cuda() ? budget() : -1;
  c.budget->host = set.host_budget > 0 ? set.host_budget : -1;
  c.dir = set.fpath;
  c.kind = "kv";
  c.instance = instance_me_;
  c.rank = comm_->rank();
  c.piece_bytes = block_bytes();
  if (budget() > 0) c.piece_bytes = std::min<int64_t>(c.piece_bytes, std::max<int64_t>(budget() / 4, 4096));
  b.set_spool(c);
}

OocEnv MapReduce::ooc_env() const {
  OocEnv e;
  e.hbm = budget();
  e.host = set.host_budget > 0 ? set.host_budget : -1;
  e.dir = set.fpath;
  e.instance = instance_me_;
  e.rank = comm_->rank();
  e.streams = set.streams;
  return e;
}

// concatenation of the KV's parts (one pass over all of them): on the
// device, or — for a bounded MR — where the budgets allow (data past the HBM
// budget is written once, to pinned host memory or one spool file)
KV MapReduce::concat_parts(const std::vector<KV>& parts) {
  if (parts.size() == 1) return parts[0];
  int64_t total = 0;
  bool on_dev = true;
  for (const KV& p : parts) {
    total += p.nbytes();
    on_dev = on_dev && p.device() == device();
  }
  if ((budget() <= 0 && set.host_budget <= 0) || !device().is_cuda() || (on_dev && (budget() <= 0 || total <= budget())))
    return concat(parts, device());
  if (set.host_budget <= 0 || total <= set.host_budget) {
    KV o = concat(parts, at::Device(at::kCPU), /*pin=*/true);  // written once, straight to pinned memory
    spool_stats.host_bytes += total;
    return o;
  }
  spool_stats.files++;
  spool_stats.disk_bytes += total;
  return kv_to_file(parts, spool_path(set.fpath, "kv", instance_me_, comm_->rank()));
}

std::vector<KMV> MapReduce::kmv_parts() const {
  std::vector<KMV> p;
  if (kmv) p.push_back(*kmv);
  for (const KMV& t : kmv_tail_) p.push_back(t);
  return p;
}

int64_t MapReduce::kmv_keys() const {
  int64_t n = kmv ? kmv->nkey : 0;
  for (const KMV& t : kmv_tail_) n += t.nkey;
  return n;
}

void MapReduce::flatten_kmv() {
  if (kmv_tail_.empty()) return;
  std::vector<KMV> parts = kmv_parts();
  kmv_tail_.clear();
  const at::Device d = parts[0].seg.device();
  kmv = kmv_concat(parts, d, d.is_cpu() && device().is_cuda());
}

void MapReduce::set_kmv_parts(std::vector<KMV> parts) {
  kmv_tail_.clear();
  kmv.reset();
  for (size_t i = 0; i < parts.size(); ++i) {
    if (i == 0) kmv = parts[0];
    else if (parts[i].nkey) kmv_tail_.push_back(parts[i]);
  }
}

void MapReduce::drop_kmv() {
  kmv.reset();
  kmv_tail_.clear();
}

std::vector<KV> MapReduce::kv_parts() const {
  std::vector<KV> p;
  if (kv) p.push_back(*kv);
  for (const KV& t : kv_tail_) p.push_back(t);
  return p;
}

int64_t MapReduce::kv_rows() const {
  int64_t n = kv ? kv->n : 0;
  for (const KV& t : kv_tail_) n += t.n;
  return n;
}

void MapReduce::flatten() {
  if (kv_tail_.empty()) return;
  std::vector<KV> parts = kv_parts();
  kv_tail_.clear();
  kv = concat_parts(parts);
  grouped_.reset();
}

void MapReduce::set_kv_parts(std::vector<KV> parts) {
  kv_tail_.clear();
  kv.reset();
  grouped_.reset();
  for (size_t i = 0; i < parts.size(); ++i) {
    if (i == 0) kv = parts[0];
    else if (parts[i].n) kv_tail_.push_back(parts[i]);
  }
}

void MapReduce::append_part(const KV& b) {
  grouped_.reset();
  if (!kv) {
    kv = b;
    return;
  }
  if (b.n == 0) return;
  KV p = b;
  if (budget() > 0 && b.device().is_cuda()) {
    int64_t on_dev = b.nbytes();
    for (const KV& x : kv_parts())
      if (x.device().is_cuda()) on_dev += x.nbytes();
    if (on_dev > budget()) {  // the new part leaves HBM through a bounded builder (its pieces only)
      KeyValue tmp(device());
      bound(tmp);
      tmp.add_kv(b);
      p = tmp.finish();
      note_spool(tmp);
    }
  }
  kv_tail_.push_back(p);
}

void MapReduce::note_spool(const KeyValue& b) {
  const SpoolStats s = b.spool_stats();
  spool_stats.add(s);
}

int64_t MapReduce::data_bytes() const {
  int64_t b = 0;
  if (kv) b += kv->nbytes();
  for (const KV& t : kv_tail_) b += t.nbytes();
  if (kmv) b += kmv->nbytes();
  for (const KMV& t : kmv_tail_) b += t.nbytes();
  return b;
}

void MapReduce::note_ooc(const char* op, const OocStats& st) {
  pages_ = std::max<int64_t>(pages_, st.parts);
  spool_stats.files += st.files;
  spool_stats.disk_bytes += st.disk_bytes;
  ooc_hot_keys += st.hot_keys;
  ooc_split_keys += st.split_keys;
  if (set.verbosity > 0 && comm_->rank() == 0)
    out(fmt("%s out of core: %" PRId64 " partitions, %" PRId64 " budget-sized chunks through HBM, %" PRId64
            " spool files\n", op, st.parts, st.chunks, st.files));
}

std::unique_ptr<MapReduce> MapReduce::copy() const {
  const_cast<MapReduce*>(this)->ensure_resident();  // a disk-resident MR copies its data, not nothing
  const_cast<MapReduce*>(this)->flatten();
  const_cast<MapReduce*>(this)->flatten_kmv();
  auto mr = std::make_unique<MapReduce>(comm_);
  mr->set = set;
  if (kv) mr->kv = clone_kv(*kv);
  if (kmv) mr->kmv = clone_kmv(*kmv);
  return mr;
}

void MapReduce::need_kv(const char* what) const {
  if (!kv) fail(std::string("Cannot ") + what + " without KeyValue");
}
void MapReduce::need_kmv(const char* what) const {
  if (!kmv) fail(std::string("Cannot ") + what + " without KeyMultiValue");
}

void MapReduce::histo(double v, const char* heading) const {
  std::vector<double> vals = comm_->allgather_f64(v);
  double ave = 0, mx = vals[0], mn = vals[0];
  for (double x : vals) {
    ave += x;
    mx = std::max(mx, x);
    mn = std::min(mn, x);
  }
  ave /= vals.size();
  int h[10] = {0};
  const double d = mx - mn;
  for (double x : vals) {
    int m = d == 0.0 ? 0 : (int)((x - mn) / d * 10.0);
    h[std::min(m, 9)]++;
  }
  if (comm_->rank() == 0) {
    std::string s = fmt("%-13s %g ave %g max %g min\n", heading, ave, mx, mn);
    s += fmt("%-13s", "  Histogram:");
    for (int i = 0; i < 10; ++i) s += fmt(" %d", h[i]);
    out(s + "\n");
  }
}

void MapReduce::note_shuffle(const ShuffleStats& st) {
  cssize += st.send_bytes;
  crsize += st.recv_bytes;
  commtime += st.seconds;
}

// ====================================================================== add / open / close

uint64_t MapReduce::add(MapReduce& other) {  // :348-374
  // O(appended): other's pairs become parts of this KV where they are (the
  // reference reopens only the last page, src/keyvalue.cpp:185-209); nothing
  // this object holds is copied
  Op frame(this, __func__, true, true);
  need_kv("add");
  other.ensure_resident();
  if (!other.kv) fail("MapReduce passed to add() does not have KeyValue pairs");
  for (const KV& p : other.kv_parts()) append_part(p);
  return frame.kv_done("Add");
}

void MapReduce::open(int addflag) {  // :1648-1664
  open_ = std::make_unique<KeyValue>(device());
  bound(*open_);
  open_add_ = addflag;
  drop_kmv();
}

KeyValue& MapReduce::kv_open() {
  if (!open_) fail("MapReduce is not open");
  return *open_;
}

uint64_t MapReduce::close() {  // :658-672
  if (!open_) fail("Cannot close MapReduce that is not open");
  Op frame(this);
  KV n = open_->finish();
  std::shared_ptr<GroupIndex> g = open_->take_group();
  open_.reset();
  if (open_add_) ensure_resident();  // appending to data that was spilled to disk
  else drop_disk();                  // replacing it: the spilled copy must never be read back over n
  if (open_add_ && kv) {
    append_part(n);
  } else {
    kv_tail_.clear();
    kv = n;
    grouped_ = g;
  }
  return frame.kv_done("Close");
}

// ====================================================================== map

std::vector<int> MapReduce::my_tasks(int nmap) {  // :1102-1225
  const int P = comm_->size(), me = comm_->rank();
  std::vector<int> t;
  if (set.mapstyle == 0 || P == 1) {
    for (int i = (int)((int64_t)me * nmap / P); i < (int)((int64_t)(me + 1) * nmap / P); ++i) t.push_back(i);
  } else if (set.mapstyle == 1) {
    for (int i = me; i < nmap; i += P) t.push_back(i);
  } else {
    // mapstyle 2: the reference dedicates rank 0 as a master handing out task
    // ids over MPI (:1164-1211); here every rank, rank 0 included, pulls the
    // next id from an atomic counter in the rendezvous store.
    static std::atomic<int64_t> ncall{0};
    comm_->barrier();
    const std::string key = "mrh_mapstyle2_" + std::to_string(instance_me_) + "_" + std::to_string(ncall++);
    for (int64_t i = comm_->next_task(key); i < nmap; i = comm_->next_task(key)) t.push_back((int)i);
    comm_->barrier();
  }
  return t;
}

// self: the KV a map over this object's own pairs read (map_mr / map_mr_batch with src == this)
uint64_t MapReduce::finish_map(Op& frame, KeyValue& kvb, int addflag, const KV* self) {
  if (self && addflag) {
    KV n = kvb.finish();
    note_spool(kvb);
    kv = *self;
    append_part(n);
    drop_kmv();
    return frame.kv_done("Map");
  }
  // the builder's chunks / spool pieces become the KV's parts (no concatenation)
  std::vector<KV> n = kvb.finish_parts();
  note_spool(kvb);
  std::shared_ptr<GroupIndex> g = kvb.take_group();
  if (addflag && kv) {
    for (const KV& p : n) append_part(p);
  } else {
    set_kv_parts(std::move(n));
    grouped_ = g;
  }
  drop_kmv();
  return frame.kv_done("Map");
}

uint64_t MapReduce::map(int nmap, const MapTaskFn& fn, int addflag) {  // :1044-1051
  Op frame(this, __func__, Op::Deferred());
  drop_for_map(addflag);
  frame.enter();
  KeyValue kvb(device());
  bound(kvb);
  for (int t : my_tasks(nmap)) fn(t, kvb);
  return finish_map(frame, kvb, addflag);
}

std::vector<std::string> MapReduce::find_files(const Comm& comm, const std::vector<std::string>& files,
                                               int selfflag, int recurse, int readflag) {  // :2812-2931
  auto local = [&]() {
    std::vector<std::string> v;
    for (auto& f : files) {
      if (readflag) {
        std::ifstream in(f);
        if (!in) fail("Could not open file " + f);
        std::string line;
        while (std::getline(in, line)) {
          std::istringstream ss(line);
          std::string w;
          if (ss >> w) expand_path(w, recurse, v);
        }
      } else {
        expand_path(f, recurse, v);
      }
    }
    return v;
  };
  if (selfflag) return local();
  std::string s = comm.rank() == 0 ? join(local()) : std::string();
  return split_lines(comm.bcast(s, 0));
}

uint64_t MapReduce::map_file(const std::vector<std::string>& files, int selfflag, int recurse, int readflag,
                             const MapFileFn& fn, int addflag) {  // :1060-1092
  Op frame(this, __func__, Op::Deferred());
  drop_for_map(addflag);
  frame.enter();
  auto fl = find_files(*comm_, files, selfflag, recurse, readflag);
  mapfilecount = (int)fl.size();
  KeyValue kvb(device());
  bound(kvb);
  if (selfflag) {
    for (int i = 0; i < (int)fl.size(); ++i) fn(i, fl[i].c_str(), kvb);
  } else {
    for (int t : my_tasks((int)fl.size())) fn(t, fl[t].c_str(), kvb);
  }
  return finish_map(frame, kvb, addflag);
}

uint64_t MapReduce::map_file_char(int nmap, const std::vector<std::string>& files, int selfflag, int recurse,
                                  int readflag, char sepchar, int delta, const MapChunkFn& fn, int addflag) {
  return map_chunks(nmap, files, selfflag, recurse, readflag, std::string(1, sepchar), true, delta, fn, addflag);
}

uint64_t MapReduce::map_file_str(int nmap, const std::vector<std::string>& files, int selfflag, int recurse,
                                 int readflag, const std::string& sepstr, int delta, const MapChunkFn& fn,
                                 int addflag) {
  return map_chunks(nmap, files, selfflag, recurse, readflag, sepstr, false, delta, fn, addflag);
}

// split files into ~nmap byte ranges, fix record boundaries with the
// separator and a `delta` look-ahead (reference map_chunks/map_file_wrapper
// :1312-1552)
uint64_t MapReduce::map_chunks(int nmap, const std::vector<std::string>& files, int selfflag, int recurse,
                               int readflag, const std::string& sep, bool is_char, int delta, const MapChunkFn& fn,
                               int addflag) {
  Op frame(this, __func__, Op::Deferred());
  drop_for_map(addflag);
  frame.enter();
  KeyValue kvb(device());
  bound(kvb);
  std::string buf;
  for_chunks(
      nmap, files, selfflag, recurse, readflag, sep, is_char, delta,
      [&](int64_t bytes) {
        buf.assign((size_t)bytes, '\0');
        return &buf[0];
      },
      [&](const FileChunk& c) {
        c.buf[c.s1] = '\0';  // the reference NUL-terminates the chunk for strtok-style callbacks
        fn(c.task, c.buf + c.s0, (int)(c.s1 - c.s0), kvb);
      });
  return finish_map(frame, kvb, addflag);
}

// The chunks of map_chunks, for the host callbacks and the device functors
// alike: the file list, the plan of ~nmap byte ranges, this rank's tasks, each
// task's read (rs bytes from st into room(rs + 1), zero-filled past what was
// read) and its boundaries s0 / s1 repaired on the separator
void MapReduce::for_chunks(int nmap, const std::vector<std::string>& files, int selfflag, int recurse, int readflag,
                           const std::string& sep, bool is_char, int delta,
                           const std::function<char*(int64_t)>& room,
                           const std::function<void(const FileChunk&)>& fn) {
  auto fl = find_files(*comm_, files, selfflag, recurse, readflag);
  mapfilecount = (int)fl.size();
  const int nfile = (int)fl.size();
  std::vector<int64_t> sizes(nfile, 0);
  if (comm_->rank() == 0 || selfflag)
    for (int i = 0; i < nfile; ++i) sizes[i] = (int64_t)std::filesystem::file_size(fl[i]);
  if (!selfflag) sizes = comm_->allreduce(sizes, Comm::SUM);
  std::vector<ChunkTask> plan;
  if (nfile) {
    nmap = std::max(nmap, nfile);
    int64_t total = std::accumulate(sizes.begin(), sizes.end(), (int64_t)0);
    int64_t ideal = std::max<int64_t>(1, total / nmap);
    std::vector<int> tpf(nfile);
    int ntasks = 0;
    for (int i = 0; i < nfile; ++i) ntasks += (tpf[i] = (int)std::max<int64_t>(1, sizes[i] / ideal));
    while (ntasks < nmap) {
      bool prog = false;
      for (int i = 0; i < nfile && ntasks < nmap; ++i)
        if (sizes[i] > ideal) {
          tpf[i]++;
          ntasks++;
          prog = true;
        }
      if (!prog) break;
    }
    while (ntasks > nmap)
      for (int i = 0; i < nfile && ntasks > nmap; ++i)
        if (tpf[i] > 1) {
          tpf[i]--;
          ntasks--;
        }
    for (int i = 0; i < nfile; ++i)
      while (tpf[i] > 1 && sizes[i] / tpf[i] <= delta) tpf[i]--;
    for (int i = 0; i < nfile; ++i)
      for (int j = 0; j < tpf[i]; ++j) plan.push_back({i, j, tpf[i], sizes[i]});
  }
  std::vector<int> tasks;
  if (selfflag) {
    tasks.resize(plan.size());
    std::iota(tasks.begin(), tasks.end(), 0);
  } else {
    tasks = my_tasks((int)plan.size());
  }
  for (int t : tasks) {
    const ChunkTask& c = plan[t];
    const int64_t st = (int64_t)c.itask * c.fsize / c.ntask, nx = (int64_t)(c.itask + 1) * c.fsize / c.ntask;
    const int64_t rs = std::min<int64_t>(nx - st + delta, c.fsize - st);
    char* b = room(rs + 1);
    std::FILE* f = std::fopen(fl[c.ifile].c_str(), "rb");
    if (!f) fail("Could not open file " + fl[c.ifile]);
    std::fseek(f, (long)st, SEEK_SET);
    size_t got = std::fread(b, 1, (size_t)rs, f);
    std::fclose(f);
    std::memset(b + got, 0, (size_t)(rs + 1) - got);
    rsize += (int64_t)got;
    const std::string_view buf(b, (size_t)rs + 1);
    int64_t s0 = 0, s1 = (int64_t)got;
    if (c.itask > 0) {
      size_t p = buf.find(sep, 0);
      if (p == std::string::npos || (int64_t)p > delta) fail("Could not find file separator within delta");
      s0 = (int64_t)p + (is_char ? (int64_t)sep.size() : 0);
    }
    if (c.itask < c.ntask - 1) {
      size_t p = buf.find(sep, (size_t)(nx - st));
      if (p == std::string::npos || (int64_t)p >= (int64_t)got) fail("Could not find file separator within delta");
      s1 = (int64_t)p + (is_char ? 1 : 0);
    }
    fn(FileChunk{t, c.ifile, st, (int64_t)got, s0, s1, b});
  }
}

uint64_t MapReduce::map_mr(MapReduce& src, const MapKVFn& fn, int addflag) {  // :1560-1642
  Op frame(this, __func__, Op::Deferred());
  drop_for_map(addflag, &src);
  frame.enter();
  src.ensure_resident();
  src.flatten();
  src.flatten_kmv();
  if (!src.kv) fail("MapReduce passed to map() does not have KeyValue pairs");
  KV s = *src.kv;
  HostCol k = host_col(s.kdata, s.koff, s.kw), v = host_col(s.vdata, s.voff, s.vw);
  align_col(k, s.n, src.set.keyalign, nullptr, 0, src.set.zeropage);
  align_col(v, s.n, src.set.valuealign, nullptr, 0, src.set.zeropage);
  KeyValue kvb(device());
  bound(kvb);
  for (int64_t i = 0; i < s.n; ++i) fn((uint64_t)i, k.at(i), (int)k.len(i), v.at(i), (int)v.len(i), kvb);
  return finish_map(frame, kvb, addflag, &src == this ? &s : nullptr);
}

uint64_t MapReduce::map_mr_batch(MapReduce& src, const MapBatchFn& fn, int addflag) {
  Op frame(this, __func__, Op::Deferred());
  drop_for_map(addflag, &src);
  frame.enter();
  src.ensure_resident();
  src.flatten();
  src.flatten_kmv();
  if (!src.kv) fail("MapReduce passed to map() does not have KeyValue pairs");
  KV s = *src.kv;
  KeyValue kvb(device());
  bound(kvb);
  fn(s, kvb);
  return finish_map(frame, kvb, addflag, &src == this ? &s : nullptr);
}

// ====================================================================== shuffle

uint64_t MapReduce::aggregate(const HashFn& hash) {  // :385-563
  Op frame(this, __func__, true, !comm_->distributed());  // one rank: nothing moves, appended parts stay
  need_kv("aggregate");
  if (comm_->distributed() && ooc_shuffle()) {
    // larger than the budget: budget-sized chunks in lock-step, received into
    // host memory (ooc.h ooc_exchange); a custom hash runs on the host first
    at::Tensor d;
    if (hash) d = host_dest(hash);
    ShuffleStats st;
    OocStats os;
    kv = ooc_exchange(*kv, d, *comm_, ooc_env(), device(), set.all2all, &os, &st);
    note_shuffle(st);
    note_ooc("Aggregate", os);
  } else if (comm_->distributed()) {
    ShuffleStats st;
    if (!hash) {
      kv = oom_retry(this, device(), my_proc(), "aggregate", [&] { return mrh::aggregate(*kv, *comm_, xopts(), &st); });
    } else {
      kv = exchange(std::move(*kv), host_dest(hash).to(device()), *comm_, xopts(), &st);
    }
    note_shuffle(st);
  }
  return frame.kv_done("Aggregate");
}

// owner rank of every pair by a user hash (MR-MPI's hash callback, run on the
// host over the KV's bytes; src/mapreduce.cpp:469-472)
at::Tensor MapReduce::host_dest(const HashFn& hash) const {
  HostCol k = host_col(kv->kdata, kv->koff, kv->kw);
  at::Tensor d = at::empty({kv->n}, at::TensorOptions().dtype(at::kInt));
  int32_t* dp = d.data_ptr<int32_t>();
  const int P = comm_->size();
  for (int64_t i = 0; i < kv->n; ++i) {
    int h = hash(k.at(i), (int)k.len(i));
    dp[i] = (int32_t)(((int64_t)h % P + P) % P);
  }
  return d;
}

// a shuffle of more than half the HBM budget on any rank streams through
// ooc_exchange on every rank (the paths' collectives differ, so the choice is
// collective: one host allreduce, and only for an MR with a budget)
bool MapReduce::ooc_shuffle() const {
  if (budget() <= 0) return false;
  const int64_t mine = kv && needs_ooc(kv->nbytes(), budget(), 2.0) ? 1 : 0;
  return comm_->allreduce(mine, Comm::MAX) != 0;
}

uint64_t MapReduce::aggregate_dest(const at::Tensor& dest) {
  Op frame(this, __func__, true, !comm_->distributed());
  need_kv("aggregate");
  if (comm_->distributed()) {
    ShuffleStats st;
    at::Tensor d = dest.to(device()).to(at::kInt).contiguous();
    if (d.numel() != kv->n) fail("aggregate: one destination per pair");
    if (d.numel()) {
      auto mm = at::aminmax(d);
      if (std::get<0>(mm).item<int>() < 0 || std::get<1>(mm).item<int>() >= comm_->size())
        fail("aggregate: destination rank out of range");
    }
    if (ooc_shuffle()) {
      OocStats os;
      kv = ooc_exchange(*kv, d.to(at::kCPU), *comm_, ooc_env(), device(), set.all2all, &os, &st);
      note_ooc("Aggregate", os);
    } else {
      kv = exchange(std::move(*kv), d, *comm_, xopts(), &st);
    }
    note_shuffle(st);
  }
  return frame.kv_done("Aggregate");
}

uint64_t MapReduce::broadcast(int root) {  // :569-623
  Op frame(this, __func__);
  need_kv("broadcast");
  if (comm_->distributed()) kv = mrh::broadcast(*kv, root, *comm_);
  return frame.kv_done("Broadcast");
}

uint64_t MapReduce::gather(int nprocs) {  // :893-1036
  Op frame(this, __func__, true);
  need_kv("gather");
  if (nprocs < 1 || nprocs > comm_->size()) fail("Invalid proc count for gather");
  if (comm_->distributed() && (nprocs < comm_->size() || comm_->uses_rccl())) {
    ShuffleStats st;
    if (ooc_shuffle()) {  // rank r's pairs to r % nprocs, budget-sized chunks into host memory
      OocStats os;
      at::Tensor d = at::full({kv->n}, comm_->rank() % nprocs, at::TensorOptions().dtype(at::kInt));
      kv = ooc_exchange(*kv, d, *comm_, ooc_env(), device(), set.all2all, &os, &st);
      note_ooc("Gather", os);
    } else {
      kv = gather_to(std::move(*kv), nprocs, *comm_, xopts(), &st);
    }
    note_shuffle(st);
  }
  return frame.kv_done("Gather");
}

// ====================================================================== group-by

namespace {
// the groups of `kv` from the index that grouped it as it arrived (grouped =
// 1), or, after a 64-bit hash collision, from an exact regroup (grouped = 2)
KMV finish_grouped(GroupIndex& g, const KV& kv, ConvertStats* cs) {
  KMV m;
  if (g.finish(&m, cs)) {
    cs->grouped = 1;
    return m;
  }
  *cs = ConvertStats();
  m = mrh::convert(kv, cs, 64);
  cs->grouped = 2;
  return m;
}
}  // namespace

uint64_t MapReduce::convert() { return convert_prehashed(at::Tensor()); }

uint64_t MapReduce::convert_prehashed(const at::Tensor& prehash) {  // :861-886
  Op frame(this, "convert", true, !prehash.defined());
  need_kv("convert");
  last_convert = ConvertStats();
  if (needs_ooc(data_bytes(), budget(), 4.0)) {
    OocStats os;
    // hash-partitioned spools (src/keymultivalue.cpp:645-789), fed from every
    // part where it lies
    set_kmv_parts(ooc_convert_parts(kv_parts(), ooc_env(), device(), &os));
    note_ooc("Convert", os);
  } else if (grouped_ && grouped_->describes(*kv) && !prehash.defined()) {
    // grouped while the map produced it: only the two short sorts are left
    kmv = finish_grouped(*grouped_, *kv, &last_convert);
  } else if (!prehash.defined() && (!kv_tail_.empty() || kv->kfixed())) {
    // narrow pairs, possibly in parts: grouped with every part read in place
    // and released once packed (packed pairs), else concatenated once for
    // the other paths
    std::vector<KV> parts = kv_parts();
    bool all_dev = true;
    for (const KV& p : parts) all_dev = all_dev && p.device() == device();
    KMV m;
    bool done = false;
    if (all_dev) {
      // the converter holds the only references: every part is freed once packed
      kv.reset();
      kv_tail_.clear();
      grouped_.reset();
      done = convert_packed_parts(parts, &m, &last_convert);
      if (!done) set_kv_parts(std::move(parts));
    }
    if (done) {
      kmv = std::move(m);
    } else {
      flatten();
      flatten_kmv();
      kmv = oom_retry(this, device(), my_proc(), "convert", [&] { return mrh::convert(*kv, &last_convert, 64); });
    }
  } else {
    kmv = oom_retry(this, device(), my_proc(), "convert",
                    [&] { return mrh::convert(*kv, &last_convert, 64, prehash); });
  }
  grouped_.reset();
  kv.reset();
  kv_tail_.clear();
  return frame.kmv_done("Convert");
}

uint64_t MapReduce::collate(const HashFn& hash) {  // :710-738
  // with a budget: aggregate and convert stream out-of-core data themselves;
  // on one rank they also read appended parts in place
  Op frame(this, __func__, true, !comm_->distributed());
  need_kv("collate");
  // pipelined collate: the hash-partition exchange hands every received round
  // to a GroupIndex, which groups it on the compute stream while the next
  // round is on the wire (alltoallv k || group k-1); the
  // group-by is done when the last round lands. MRH_PIPELINE_COLLATE=0 turns
  // it off; out-of-core data (an HBM budget in force) keeps aggregate+convert.
  static const bool pipeline_env = [] {
    const char* e = std::getenv("MRH_PIPELINE_COLLATE");
    return !(e && *e == '0');
  }();
  const bool pipeline = set.pipeline < 0 ? pipeline_env : set.pipeline != 0;
  if (pipeline && !hash && comm_->distributed() && budget() == 0) {
    ShuffleStats st;
    GroupIndex g(device());
    ExchangeOpts o = xopts();
    o.round_sink = [&](const KV& r) { g.add(r); };
    KV rest = exchange(std::move(*kv), at::Tensor(), *comm_, o, &st);
    note_shuffle(st);
    last_convert = ConvertStats();
    if (g.size() == 0) {
      kv = rest;
      kmv = mrh::convert(*kv, &last_convert);
    } else {
      kv = g.kv();
      kmv = finish_grouped(g, *kv, &last_convert);
    }
    kv.reset();
    grouped_.reset();
    return frame.kmv_done("Collate");
  }
  {
    Quiet quiet(set);
    aggregate(hash);
    convert();
  }
  return frame.kmv_done("Collate");
}

// compress's local group-by: out of core (hash-partitioned spools) past the budget
KMV MapReduce::local_groups(const char* heading) {
  last_convert = ConvertStats();
  if (needs_ooc(kv->nbytes(), budget(), 4.0)) {
    OocStats os;
    KMV m = ooc_convert({*kv}, ooc_env(), device(), &os);
    note_ooc(heading, os);
    return m;
  }
  return mrh::convert(*kv, &last_convert);
}

uint64_t MapReduce::clone() {  // :631-652
  Op frame(this, __func__, true);  // one value per key: a host-resident KV is cloned where it lives
  need_kv("clone");
  kmv = oom_retry(this, device(), my_proc(), "clone", [&] { return mrh::clone(*kv); });
  kv.reset();
  return frame.kmv_done("Clone");
}

uint64_t MapReduce::collapse(const char* key, int kb) {  // :681-702
  Op frame(this, __func__);
  need_kv("collapse");
  kmv = mrh::collapse(*kv, std::string(key, (size_t)kb));
  kv.reset();
  return frame.kmv_done("Collapse");
}

uint64_t MapReduce::scrunch(int nprocs, const char* key, int kb) {  // :2075-2095
  Op frame(this, __func__);
  {
    Quiet quiet(set);
    gather(nprocs);
    collapse(key, kb);
  }
  return frame.kmv_done("Scrunch");
}

// ====================================================================== reduce family

namespace {
// the value type of the builtin reducers when the caller names none
const std::string& builtin_dtype(const std::string& dtype) {
  static const std::string int32 = "int32";
  return dtype.empty() ? int32 : dtype;
}
}  // namespace

ExchangeOpts MapReduce::xopts() const {
  ExchangeOpts o;
  o.chunk_bytes = set.chunk_bytes > 0 ? set.chunk_bytes : 2 * block_bytes();
  o.hbm_budget = budget();
  o.all2all = set.all2all;
  return o;
}

int64_t MapReduce::budget() const {
  if (set.hbm_budget > 0) return set.hbm_budget;
  if (set.maxpage > 0) return (int64_t)set.maxpage * block_bytes();
  return 0;
}

int64_t MapReduce::block_bytes() const {
  // one "page" of values per host block: memsize MB (negative = bytes)
  return set.memsize > 0 ? (int64_t)set.memsize << 20 : std::max<int64_t>(512, -(int64_t)set.memsize);
}

// Drive a host callback over every KMV pair. Keys whose values exceed one page
// use the reference's multi-block protocol (:1828-1848): mv == nullptr,
// nvalues == 0, valuebytes == (int*)this, then multivalue_blocks/_block.
void MapReduce::run_host_kmv(const KMV& m, const std::function<void(char*, int, char*, int, int*)>& fn) {
  HostCol k = host_col(m.keys.kdata, m.keys.koff, m.keys.kw), v = host_col(m.vdata, m.voff, m.vw);
  at::Tensor seg = m.seg.to(at::kCPU).contiguous();
  const int64_t* s = seg.data_ptr<int64_t>();
  align_col(k, m.nkey, set.keyalign, nullptr, 0, set.zeropage);
  align_col(v, m.nval, set.valuealign, s, m.nkey, set.zeropage);
  std::vector<int> vsz((size_t)m.nval);
  for (int64_t j = 0; j < m.nval; ++j) vsz[j] = (int)v.len(j);
  const int64_t page = block_bytes();
  for (int64_t i = 0; i < m.nkey; ++i) {
    const int64_t a = s[i], b = s[i + 1];
    char* mv = v.at(a);
    const int64_t mvbytes = b > a ? v.a(b - 1) + v.len(b - 1) - v.a(a) : 0;
    if (mvbytes <= page || b - a <= 1) {
      fn(k.at(i), (int)k.len(i), mv ? mv : k.at(i), (int)(b - a), vsz.data() + a);
      continue;
    }
    blk_.mv = mv;
    blk_.sizes = vsz.data() + a;
    blk_.nval = b - a;
    blk_.start.clear();
    blk_.boff.clear();
    int64_t acc = 0, off = 0;
    for (int64_t j = 0; j < b - a; ++j) {
      if (j == 0 || acc + vsz[a + j] > page) {
        blk_.start.push_back(j);
        blk_.boff.push_back(off);
        acc = 0;
      }
      acc += vsz[a + j];
      off += vsz[a + j];
    }
    blk_.start.push_back(b - a);
    fn(k.at(i), (int)k.len(i), nullptr, 0, reinterpret_cast<int*>(this));
    blk_ = Blocks();
  }
}

uint64_t MapReduce::multivalue_blocks(int& nblock) const {
  nblock = blk_.start.empty() ? 0 : (int)blk_.start.size() - 1;
  return (uint64_t)blk_.nval;
}

int MapReduce::multivalue_block(int iblock, char** mv, int** valuebytes) {
  if (iblock < 0 || iblock + 1 >= (int)blk_.start.size()) fail("Invalid page request for multivalue_block");
  const int64_t j0 = blk_.start[iblock], j1 = blk_.start[iblock + 1];
  *mv = blk_.mv + blk_.boff[iblock];
  *valuebytes = const_cast<int*>(blk_.sizes + j0);
  return (int)(j1 - j0);
}

// The body of the host / batch reduce and compress ops: `fn(groups, builder)`
// emits into a bounded builder whose parts become the KV. It sees each KMV of
// `src` whole or, with `pieces`, as key ranges whose values fit the budget,
// in HBM one at a time (each a KMV of its own, in key order).
template <typename Fn>
void MapReduce::emit_kv(const std::vector<KMV>& src, bool pieces, const char* heading, Fn&& fn) {
  KeyValue kvb(device());
  bound(kvb);
  if (pieces) {
    OocStats os;
    for (const KMV& m : src)
      ooc_for_each_kmv_piece(m, ooc_env(), device(), [&](const KMV& piece) { fn(piece, kvb); }, &os);
    note_ooc(heading, os);
  } else {
    for (const KMV& m : src) fn(m, kvb);
  }
  set_kv_parts(kvb.finish_parts());
  note_spool(kvb);
}
// the host callback form: every group where it lies, never in pieces
void MapReduce::emit_kv(const std::vector<KMV>& src, const ReduceFn& fn) {
  emit_kv(src, false, nullptr, [&](const KMV& m, KeyValue& kvb) {
    run_host_kmv(m, [&](char* k, int kb, char* mv, int nv, int* vb) { fn(k, kb, mv, nv, vb, kvb); });
  });
}

uint64_t MapReduce::reduce(const ReduceFn& fn) {  // :1769-1867
  Op frame(this, __func__, true, false, true);  // host callbacks read host-resident data (every KMV part) in place
  need_kmv("reduce");
  emit_kv(kmv_parts(), fn);
  drop_kmv();
  return frame.kv_done("Reduce");
}

uint64_t MapReduce::reduce_builtin(const std::string& op, const std::string& dtype) {
  Op frame(this, __func__, true, false, kmv_part_count() > 1);
  need_kmv("reduce");
  const std::string& dt = builtin_dtype(dtype);
  if (kmv_part_count() > 1 && budget() <= 0) {
    // parts left by an out-of-core convert, but no budget now (it was lowered
    // to 0 = unlimited): each part reduced whole on the engine device (the
    // block path would cut pieces of env.hbm / 4 = 1 byte)
    std::vector<KV> outs;
    for (const KMV& m : kmv_parts()) {
      const KMV dm = m.seg.device() == device() ? m : kmv_to(m, device(), false);
      outs.push_back(oom_retry(this, device(), my_proc(), "reduce_builtin",
                               [&] { return mrh::reduce_builtin(dm, op, dt); }));
    }
    set_kv_parts(std::move(outs));
  } else if (kmv_part_count() > 1 || needs_ooc(kmv->nbytes(), budget(), 2.0)) {
    // values stream through HBM in budget-sized key ranges, part by part
    OocStats os;
    std::vector<KV> outs;
    for (const KMV& m : kmv_parts()) outs.push_back(ooc_reduce_builtin(m, op, dt, ooc_env(), device(), &os));
    set_kv_parts(std::move(outs));
    note_ooc("Reduce", os);
  } else {
    kv = oom_retry(this, device(), my_proc(), "reduce_builtin",
                   [&] { return mrh::reduce_builtin(*kmv, op, dt); });
  }
  drop_kmv();
  return frame.kv_done("Reduce");
}

uint64_t MapReduce::reduce_batch(const ReduceBatchFn& fn) {
  Op frame(this, __func__, true, false, kmv_part_count() > 1);
  need_kmv("reduce");
  emit_kv(kmv_parts(), kmv_part_count() > 1 || needs_ooc(kmv->nbytes(), budget(), 2.0), "Reduce", fn);
  drop_kmv();
  return frame.kv_done("Reduce");
}

uint64_t MapReduce::compress(const ReduceFn& fn) {  // :749-851
  Op frame(this, __func__, true);  // host callbacks read the (host-resident) groups in place
  need_kv("compress");
  emit_kv({local_groups("Compress")}, fn);
  return frame.kv_done("Compress");
}

// compress with a batch callback: the local groups of this rank's pairs as one
// KMV (pieces of it when they exceed the budget), fn emits tensors — the
// combiner form of reduce_batch (reference compress, src/mapreduce.cpp:749-851)
uint64_t MapReduce::compress_batch(const ReduceBatchFn& fn) {
  Op frame(this, __func__, true);
  need_kv("compress");
  const KMV m = local_groups("Compress");
  emit_kv({m}, needs_ooc(m.nbytes(), budget(), 2.0) || (device().is_cuda() && !m.seg.is_cuda()), "Compress", fn);
  return frame.kv_done("Compress");
}

// ====================================================================== device functors

namespace {
// items per functor launch: all of them, unless the builder is bounded (out
// of core): then about a spool piece's worth (the count / scan scratch and the
// output take ~128 bytes per item), so the launch fits the HBM budget
int64_t functor_chunk(const KeyValue& out, int64_t n) {
  const int64_t pb = out.piece_bytes();
  return pb > 0 ? std::max<int64_t>(4096, pb / 128) : std::max<int64_t>(n, 1);
}
// reduce_device / compress_device: the groups a batch op hands over, through the functor
ReduceBatchFn functor_reduce(const std::string& code, at::Device dev, const devfn::Args& bound) {
  return [=](const KMV& m, KeyValue& out) {
    if (!m.nkey) return;
    KV o = devfn::reduce_groups(m, code, dev, bound);
    if (o.n) out.add_kv(o);
  };
}
}  // namespace

void MapReduce::set_device_args(std::vector<at::Tensor> bufs) {
  if ((int)bufs.size() > devfn::kMaxArgs)
    fail("mrhip: set_device_args: at most " + std::to_string(devfn::kMaxArgs) + " device buffers can be bound, " +
         std::to_string(bufs.size()) + " given (argument " + std::to_string(devfn::kMaxArgs) + " is one too many)");
  const at::Device dev = device();
  for (size_t i = 0; i < bufs.size(); ++i) {
    const std::string which = "mrhip: set_device_args: argument " + std::to_string(i);
    const at::Tensor& t = bufs[i];
    if (!t.defined()) fail(which + " is not a defined tensor");
    if (!t.is_contiguous()) fail(which + " is not contiguous");
    const bool same = t.device().type() == dev.type() &&
                      (!dev.is_cuda() || !dev.has_index() || t.device().index() == dev.index());
    if (!same) fail(which + " is on " + t.device().str() + ", this MapReduce's device is " + dev.str());
  }
  dev_args_ = std::move(bufs);
}

uint64_t MapReduce::map_device(MapReduce& src, const std::string& code, int addflag) {
  const at::Device dev = device();
  const devfn::Args bound = devfn::args_of(dev_args_);
  return map_mr_batch(
      src,
      [&](const KV& kv, KeyValue& out) {
        if (!kv.n) return;
        const KV d = kv.device() == dev ? kv : kv_to(kv, dev);
        const int64_t step = functor_chunk(out, d.n);
        for (int64_t a = 0; a < d.n; a += step) {
          KV o = devfn::map_pairs(d, code, dev, a, std::min(d.n, a + step), bound);
          if (o.n) out.add_kv(o);
        }
      },
      addflag);
}

uint64_t MapReduce::map_device_tasks(int64_t ntask, const std::string& code, int addflag) {
  // one map task per rank-sized range of the ntask items: task t runs
  // [t * ntask / P, (t + 1) * ntask / P) in one launch (any mapstyle)
  const int64_t P = comm_->size();
  const at::Device dev = device();
  const devfn::Args bound = devfn::args_of(dev_args_);
  return map(
      (int)P,
      [&](int t, KeyValue& out) {
        const int64_t a = (int64_t)t * ntask / P, b = (int64_t)(t + 1) * ntask / P;
        const int64_t step = functor_chunk(out, b - a);
        for (int64_t x = a; x < b; x += step) {
          KV o = devfn::map_tasks(x, std::min(b, x + step) - x, code, dev, bound);
          if (o.n) out.add_kv(o);
        }
      },
      addflag);
}

uint64_t MapReduce::map_file_char_device(int nmap, const std::vector<std::string>& files, int selfflag, int recurse,
                                         int readflag, char sepchar, int delta, const std::string& code, int addflag) {
  return map_chunks_device(nmap, files, selfflag, recurse, readflag, std::string(1, sepchar), true, delta, code,
                           addflag);
}

uint64_t MapReduce::map_file_str_device(int nmap, const std::vector<std::string>& files, int selfflag, int recurse,
                                        int readflag, const std::string& sepstr, int delta, const std::string& code,
                                        int addflag) {
  return map_chunks_device(nmap, files, selfflag, recurse, readflag, sepstr, false, delta, code, addflag);
}

// map_chunks with a device functor over the chunk's records: every task's
// chunk is read into pinned host memory, copied to HBM once, cut into records
// there (split_records) and mapped in place (devfn::map_records). The records
// do not depend on where the chunks were cut: a chunk boundary is an
// occurrence of the separator, and every occurrence bounds a record.
uint64_t MapReduce::map_chunks_device(int nmap, const std::vector<std::string>& files, int selfflag, int recurse,
                                      int readflag, const std::string& sep, bool is_char, int delta,
                                      const std::string& code, int addflag) {
  constexpr int64_t kPad = 32;  // readable bytes past the text (split_records)
  if (sep.empty() || sep.size() > 16)
    fail("mrhip: a device file map splits on a separator of 1 to 16 bytes, " + std::to_string(sep.size()) + " given");
  const at::Device dev = device();
  if (!dev.is_cuda()) fail("mrhip: device functors run on a GPU MapReduce (device cuda)");
  const devfn::Args args = devfn::args_of(dev_args_);
  Op frame(this, __func__, Op::Deferred());
  drop_for_map(addflag);
  frame.enter();
  KeyValue out(dev);
  bound(out);
  const int64_t L = (int64_t)sep.size();
  at::Tensor host;  // one pinned buffer, grown as needed: every task is done with it before the next read
  for_chunks(
      nmap, files, selfflag, recurse, readflag, sep, is_char, delta,
      [&](int64_t bytes) {
        if (!host.defined() || host.numel() < bytes + kPad) host = hostarena::pinned_empty({bytes + kPad}, at::kByte);
        std::memset(host.data_ptr<uint8_t>() + bytes, 0, (size_t)kPad);
        return reinterpret_cast<char*>(host.data_ptr<uint8_t>());
      },
      [&](const FileChunk& c) {
        const int64_t n = c.s1 - c.s0;
        if (n <= 0) return;
        const int64_t nread = std::min<int64_t>(c.got - c.s0, n + L - 1);
        note_xfer_bytes(true, nread + kPad);
        const at::Tensor text = to_device(host.narrow(0, c.s0, nread + kPad), dev, /*non_blocking=*/true);
        // (split_records reads its counts back on this stream: the copy has left the pinned buffer by then)
        auto [off, nrec] = split_records(text, n, nread, sep, is_char);
        const int64_t step = functor_chunk(out, nrec);
        for (int64_t a = 0; a < nrec; a += step) {
          KV o = devfn::map_records(text, off, nrec, is_char ? 1 : 0, c.ifile, c.st + c.s0, code, dev, a,
                                    std::min(nrec, a + step), args);
          if (o.n) out.add_kv(o);
        }
      });
  return finish_map(frame, out, addflag);
}

uint64_t MapReduce::reduce_device(const std::string& code) {
  return reduce_batch(functor_reduce(code, device(), devfn::args_of(dev_args_)));
}

namespace {
// what the sorts of one column report: the op name (trace, fault points,
// errors) and the stats heading
const char* sort_name(bool by_value) { return by_value ? "sort_values" : "sort_keys"; }
const char* sort_heading(bool by_value) { return by_value ? "Sort_values" : "Sort_keys"; }

// the values of a KMV reordered by an int32 permutation (within each key's
// segment): fixed-width rows, or variable-width ones with their new offsets
void permute_values(KMV& m, const at::Tensor& perm) {
  at::Tensor noff;
  m.vdata = gather_rows(m.vdata, m.voff, m.vw, perm, m.vw < 0 ? &noff : nullptr);
  if (m.vw < 0) m.voff = noff;
}

// the pairs sorted by a device sort functor over one column, stable:
// mr_sortkey -> radix sort of its 64-bit keys; mr_compare -> the merge sort
KV sort_by_functor(const KV& kv_in, const std::string& code, int bits, bool by_value, at::Device dev,
                   const devfn::Args& bound) {
  const devfn::Kind kind = devfn::sort_kind_of(code);
  if (kv_in.n <= 1) return kv_in;
  const KV kv = kv_in.device() == dev ? kv_in : kv_to(kv_in, dev);
  const at::Tensor& data = by_value ? kv.vdata : kv.kdata;
  const at::Tensor& off = by_value ? kv.voff : kv.koff;
  const int w = by_value ? kv.vw : kv.kw;
  if (kind == devfn::Kind::Compare)
    return gather(kv, devfn::compare_perm(data, off, w, kv.n, at::Tensor(), code, dev, bound));
  auto [key, idx] = devfn::sort_keys_of(data, off, w, kv.n, code, dev, bound);
  auto [ks, perm, passes] = radix_sort_pairs(key, idx, 0, std::max(1, std::min(bits, 64)));
  (void)ks;
  (void)passes;
  return gather(kv, perm);
}
}  // namespace

// sort_keys_device / sort_values_device: the trace and the fault points see
// the op's own name, need_kv and the heading those of sort_keys / sort_values
uint64_t MapReduce::sort_column_device(bool by_value, const std::string& code, int bits) {
  Op frame(this, by_value ? "sort_values_device" : "sort_keys_device");
  need_kv(sort_name(by_value));
  kv = sort_by_functor(*kv, code, bits, by_value, device(), devfn::args_of(dev_args_));
  return frame.kv_done(sort_heading(by_value));
}

uint64_t MapReduce::sort_keys_device(const std::string& code, int bits) {
  return sort_column_device(false, code, bits);
}

uint64_t MapReduce::sort_values_device(const std::string& code, int bits) {
  return sort_column_device(true, code, bits);
}

uint64_t MapReduce::sort_multivalues_device(const std::string& code, int bits) {
  Op frame(this, "sort_multivalues");
  need_kmv("sort_multivalues");
  const devfn::Kind kind = devfn::sort_kind_of(code);
  const at::Device dev = device();
  const devfn::Args bound = devfn::args_of(dev_args_);
  if (kmv->nval > 1) {
    KMV m = kmv->seg.device() == dev ? *kmv : kmv_to(*kmv, dev, false);
    at::Tensor perm;
    if (kind == devfn::Kind::Compare) {
      // the values are grouped by key already: one sort under (segment id, mr_compare)
      perm = devfn::compare_perm(m.vdata, m.voff, m.vw, m.nval, segment_ids(m.seg, m.nkey, m.nval), code, dev,
                                 bound);
    } else {
      // LSD, as mrh::sort_multivalues: stable by the functor's key, then stable by segment id
      auto [key, idx] = devfn::sort_keys_of(m.vdata, m.voff, m.vw, m.nval, code, dev, bound);
      auto [ks, perm1, p1] = radix_sort_pairs(key, idx, 0, std::max(1, std::min(bits, 64)));
      at::Tensor sid_p = segment_ids(m.seg, m.nkey, m.nval).index_select(0, perm1.to(at::kLong));
      auto [ss, perm2, p2] = radix_sort_pairs(sid_p, perm1, 0, 64);
      (void)ks;
      (void)ss;
      (void)p1;
      (void)p2;
      perm = perm2;
    }
    permute_values(m, perm);
    kmv = m;
  }
  return frame.kmv_done("Sort_multivalues");
}

uint64_t MapReduce::compress_device(const std::string& code) {
  return compress_batch(functor_reduce(code, device(), devfn::args_of(dev_args_)));
}

// scan with a device functor: the data stays where and as it is. Pairs /
// groups in HBM take one launch; host-resident data (past the HBM budget)
// goes through HBM in budget-sized pieces, every item once, a pair's index
// its index on this rank.
uint64_t MapReduce::scan_device(const std::string& code) {
  Op frame(this, __func__, Op::Deferred());
  const at::Device dev = device();
  if (!dev.is_cuda()) fail("mrhip: device functors run on a GPU MapReduce (device cuda)");
  const devfn::Args bound = devfn::args_of(dev_args_);
  frame.enter(true, false, true);
  if (kv) {
    if (kv->n && !kv->device().is_cuda()) {
      OocStats os;
      ooc_for_each_kv_piece(*kv, ooc_env(), dev,
                            [&](const KV& piece, int64_t first) { devfn::scan_pairs(piece, first, code, dev, bound); }, &os);
      note_ooc("Scan", os);
    } else if (kv->n) {
      devfn::scan_pairs(*kv, 0, code, dev, bound);
    }
    return frame.kv_done("Scan");
  }
  need_kmv("scan");
  OocStats os;
  bool pieces = false;
  for (const KMV& m : kmv_parts()) {
    if (!m.nkey) continue;
    if (!m.seg.is_cuda() || needs_ooc(m.nbytes(), budget(), 2.0)) {
      pieces = true;
      ooc_for_each_kmv_piece(m, ooc_env(), dev, [&](const KMV& piece) { devfn::scan_groups(piece, code, dev, bound); },
                             &os);
    } else {
      devfn::scan_groups(m, code, dev, bound);
    }
  }
  if (pieces) note_ooc("Scan", os);
  return frame.kmv_done("Scan");
}

uint64_t MapReduce::compress_builtin(const std::string& op, const std::string& dtype) {
  Op frame(this, __func__, true);
  need_kv("compress");
  const std::string& dt = builtin_dtype(dtype);
  KMV m = local_groups("Compress");
  if (needs_ooc(m.nbytes(), budget(), 2.0)) {
    OocStats os;
    kv = ooc_reduce_builtin(m, op, dt, ooc_env(), device(), &os);
    note_ooc("Compress", os);
  } else {
    kv = mrh::reduce_builtin(m, op, dt);
  }
  return frame.kv_done("Compress");
}

uint64_t MapReduce::scan_kv(const ScanKVFn& fn) {  // :1933-1976
  Op frame(this, __func__, true);  // host callbacks read host-resident data in place
  need_kv("scan");
  HostCol k = host_col(kv->kdata, kv->koff, kv->kw), v = host_col(kv->vdata, kv->voff, kv->vw);
  align_col(k, kv->n, set.keyalign, nullptr, 0, set.zeropage);
  align_col(v, kv->n, set.valuealign, nullptr, 0, set.zeropage);
  for (int64_t i = 0; i < kv->n; ++i) fn(k.at(i), (int)k.len(i), v.at(i), (int)v.len(i));
  return frame.kv_done("Scan");
}

uint64_t MapReduce::scan_kmv(const ScanKMVFn& fn) {  // :1984-2065
  Op frame(this, __func__, true, false, true);  // host callbacks read host-resident data (every KMV part) in place
  need_kmv("scan");
  for (const KMV& m : kmv_parts()) run_host_kmv(m, fn);
  return frame.kmv_done("Scan");
}

// ====================================================================== sorting

namespace {
// host stable sort of one column with a user comparator -> device int32 perm
at::Tensor host_perm(const at::Tensor& data, const at::Tensor& off, int w, int64_t n, const CompareFn& fn,
                     at::Device dev) {
  HostCol c = host_col(data, off, w);
  std::vector<int32_t> p((size_t)n);
  std::iota(p.begin(), p.end(), 0);
  std::stable_sort(p.begin(), p.end(),
                   [&](int32_t a, int32_t b) { return fn(c.at(a), (int)c.len(a), c.at(b), (int)c.len(b)) < 0; });
  return at::from_blob(p.data(), {n}, at::TensorOptions().dtype(at::kInt)).clone().to(dev);
}
}  // namespace

// sort_keys / sort_values (reference :2102-2203): one column, by a type flag or a host comparator
uint64_t MapReduce::sort_column(bool by_value, int flag) {
  const char* name = sort_name(by_value);
  Op frame(this, name, true);
  need_kv(name);
  if (needs_ooc(kv->nbytes(), budget(), 4.0)) {
    OocStats os;
    kv = ooc_sort(*kv, flag, by_value, ooc_env(), device(), &os);  // sample sort over host spools
    note_ooc(sort_heading(by_value), os);
  } else {
    kv = oom_retry(this, device(), my_proc(), name, [&] { return sort_kv(*kv, flag, by_value); });
  }
  return frame.kv_done(sort_heading(by_value));
}
uint64_t MapReduce::sort_column(bool by_value, const CompareFn& fn) {
  Op frame(this, sort_name(by_value));
  need_kv(sort_name(by_value));
  if (kv->n > 1)
    kv = mrh::gather(*kv, host_perm(by_value ? kv->vdata : kv->kdata, by_value ? kv->voff : kv->koff,
                                    by_value ? kv->vw : kv->kw, kv->n, fn, device()));
  return frame.kv_done(sort_heading(by_value));
}
uint64_t MapReduce::sort_keys(int flag) { return sort_column(false, flag); }
uint64_t MapReduce::sort_keys(const CompareFn& fn) { return sort_column(false, fn); }
uint64_t MapReduce::sort_values(int flag) { return sort_column(true, flag); }
uint64_t MapReduce::sort_values(const CompareFn& fn) { return sort_column(true, fn); }

uint64_t MapReduce::sort_multivalues(int flag) {  // :2210-2352
  Op frame(this, __func__);
  need_kmv("sort_multivalues");
  kmv = mrh::sort_multivalues(*kmv, flag);
  return frame.kmv_done("Sort_multivalues");
}
uint64_t MapReduce::sort_multivalues(const CompareFn& fn) {
  Op frame(this, __func__);
  need_kmv("sort_multivalues");
  KMV& m = *kmv;
  HostCol v = host_col(m.vdata, m.voff, m.vw);
  at::Tensor seg = m.seg.to(at::kCPU).contiguous();
  const int64_t* s = seg.data_ptr<int64_t>();
  std::vector<int32_t> p((size_t)m.nval);
  std::iota(p.begin(), p.end(), 0);
  for (int64_t i = 0; i < m.nkey; ++i)
    std::stable_sort(p.begin() + s[i], p.begin() + s[i + 1], [&](int32_t a, int32_t b) {
      return fn(v.at(a), (int)v.len(a), v.at(b), (int)v.len(b)) < 0;
    });
  permute_values(m, at::from_blob(p.data(), {m.nval}, at::TensorOptions().dtype(at::kInt)).clone().to(device()));
  return frame.kmv_done("Sort_multivalues");
}

// ====================================================================== print

void MapReduce::print(int proc, int nstride, int kflag, int vflag) { print(nullptr, 0, proc, nstride, kflag, vflag); }

void MapReduce::print(const char* file, int fflag, int proc, int nstride, int kflag, int vflag) {
  ensure_resident();
  flatten();
  flatten_kmv();
  if (!kv && !kmv) fail("Cannot print without KeyValue or KeyMultiValue");
  if (kflag < 0 || kflag > 7 || vflag < 0 || vflag > 7 || nstride < 1) fail("Invalid print args");
  const int me = comm_->rank();
  std::string text;
  int cnt = 0;
  if (kv) {
    HostCol k = host_col(kv->kdata, kv->koff, kv->kw), v = host_col(kv->vdata, kv->voff, kv->vw);
    for (int64_t i = 0; i < kv->n; ++i) {
      if (++cnt != nstride) continue;
      cnt = 0;
      text += fmt("KV pair: proc %d, sizes %d %d, key ", me, (int)k.len(i), (int)v.len(i)) +
              fmt_item(k.at(i), k.len(i), kflag) + ", value " + fmt_item(v.at(i), v.len(i), vflag) + "\n";
    }
  } else {
    HostCol k = host_col(kmv->keys.kdata, kmv->keys.koff, kmv->keys.kw), v = host_col(kmv->vdata, kmv->voff, kmv->vw);
    at::Tensor seg = kmv->seg.to(at::kCPU).contiguous();
    const int64_t* s = seg.data_ptr<int64_t>();
    for (int64_t i = 0; i < kmv->nkey; ++i) {
      if (++cnt != nstride) continue;
      cnt = 0;
      int64_t mvb = 0;
      std::string vs;
      for (int64_t j = s[i]; j < s[i + 1]; ++j) {
        mvb += v.len(j);
        if (vflag) vs += fmt_item(v.at(j), v.len(j), vflag) + " ";
      }
      if (!vflag) vs = "NULL";
      text += fmt("KMV pair: proc %d, nvalues %d, sizes %d %d, key ", me, (int)(s[i + 1] - s[i]), (int)k.len(i),
                  (int)mvb) +
              fmt_item(k.at(i), k.len(i), kflag) + ", values " + vs + "\n";
    }
  }
  write_text(file, fflag, proc, [&](const TextSink& sink) { sink(text.data(), text.size()); });
}

void MapReduce::write_text(const char* file, int fflag, int proc, const std::function<void(const TextSink&)>& body) {
  const int me = comm_->rank();
  auto emit = [&](const char* path, const char* mode) {
    if (!path) {
      body([](const char* b, size_t n) { out(std::string(b, n)); });
      return;
    }
    std::unique_ptr<std::FILE, int (*)(std::FILE*)> f(std::fopen(path, mode), &std::fclose);
    if (!f) fail(std::string("Could not open print file ") + path);
    body([&](const char* b, size_t n) {
      std::fwrite(b, 1, n, f.get());
      wsize += (int64_t)n;
    });
  };
  if (proc >= 0) {
    if (proc == me) emit(file, "w");
    return;
  }
  if (file && fflag == 1) {
    std::string p = std::string(file) + "." + std::to_string(me);
    emit(p.c_str(), "w");
    return;
  }
  // token ring: ranks print in order (reference :1696-1709)
  if (file && me == 0) emit(file, "w");
  for (int r = 0; r < comm_->size(); ++r) {
    comm_->barrier();
    if (r == me && !(file && me == 0)) emit(file, "a");
  }
  comm_->barrier();
}

// print with a device functor: pairs / groups in HBM are formatted by one
// launch pair; host-resident data (past the HBM budget) goes through HBM in
// budget-sized pieces as for scan_device, a pair's index its index on this
// rank. The data stays where and as it is.
void MapReduce::for_each_text(const std::string& code, const std::function<void(const at::Tensor&)>& fn) {
  const at::Device dev = device();
  const devfn::Args bound = devfn::args_of(dev_args_);
  if (kv) {
    if (kv->n && !kv->device().is_cuda()) {
      OocStats os;
      ooc_for_each_kv_piece(*kv, ooc_env(), dev,
                            [&](const KV& piece, int64_t first) { fn(devfn::format_pairs(piece, first, code, dev, bound)); },
                            &os);
      note_ooc("Print", os);
    } else {
      fn(devfn::format_pairs(*kv, 0, code, dev, bound));
    }
    return;
  }
  need_kmv("print");
  OocStats os;
  bool pieces = false;
  for (const KMV& m : kmv_parts()) {
    if (!m.nkey) continue;
    if (!m.seg.is_cuda() || needs_ooc(m.nbytes(), budget(), 2.0)) {
      pieces = true;
      ooc_for_each_kmv_piece(m, ooc_env(), dev,
                             [&](const KMV& piece) { fn(devfn::format_groups(piece, code, dev, bound)); }, &os);
    } else {
      fn(devfn::format_groups(m, code, dev, bound));
    }
  }
  if (pieces) note_ooc("Print", os);
}

at::Tensor MapReduce::text_device(const std::string& code) {
  Op frame(this, __func__, Op::Deferred());
  const at::Device dev = device();
  if (!dev.is_cuda()) fail("mrhip: device functors run on a GPU MapReduce (device cuda)");
  frame.enter(true, false, true);
  if (!kv) need_kmv("print");
  devfn::load_print(code, !kv, dev);
  std::vector<at::Tensor> texts;
  for_each_text(code, [&](const at::Tensor& t) {
    if (t.numel()) texts.push_back(t);
  });
  if (kv) frame.kv_done("Text");
  else frame.kmv_done("Text");
  if (texts.empty()) return at::empty({0}, at::TensorOptions().device(dev).dtype(at::kByte));
  return texts.size() == 1 ? texts[0] : at::cat(texts);
}

uint64_t MapReduce::print_device(const char* file, int fflag, int proc, const std::string& code) {
  Op frame(this, __func__, Op::Deferred());
  if (!device().is_cuda()) fail("mrhip: device functors run on a GPU MapReduce (device cuda)");
  frame.enter(true, false, true);
  if (!kv) need_kmv("print");
  devfn::load_print(code, !kv, device());
  // a piece's text reaches the sink through pinned host memory, at most kHostText bytes at a time
  constexpr int64_t kHostText = int64_t(64) << 20;
  at::Tensor host;
  int64_t written = 0;
  write_text(file, fflag, proc, [&](const TextSink& sink) {
    for_each_text(code, [&](const at::Tensor& t) {
      for (int64_t a = 0; a < t.numel(); a += kHostText) {
        const int64_t n = std::min<int64_t>(kHostText, t.numel() - a);
        if (!host.defined() || host.numel() < n) host = hostarena::pinned_empty({n}, at::kByte);
        host.narrow(0, 0, n).copy_(t.narrow(0, a, n));  // not non_blocking: complete on return
        sink(reinterpret_cast<const char*>(host.data_ptr()), (size_t)n);
        written += n;
      }
    });
  });
  if (kv) frame.kv_done("Print");
  else frame.kmv_done("Print");
  return count(written);
}

// ====================================================================== stats

uint64_t MapReduce::kv_stats(int level) {  // :2937-2966
  ensure_resident();
  flatten();
  flatten_kmv();
  need_kv("print stats");
  std::vector<int64_t> t =
      comm_->allreduce({kv->n, kv->key_bytes(), kv->value_bytes(), kv->nbytes(), pages(kv->nbytes())}, Comm::SUM);
  const double mb = 1024.0 * 1024.0;
  if (level == 1 && comm_->rank() == 0)
    out(fmt("%" PRId64 " pairs, %.3g Mb keys, %.3g Mb values, %.3g Mb, %" PRId64 " pages\n", t[0], t[1] / mb,
            t[2] / mb, t[3] / mb, t[4]));
  if (level == 2) {
    histo((double)kv->n, "  KV pairs:");
    histo(kv->key_bytes() / mb, "  Kdata (Mb):");
    histo(kv->value_bytes() / mb, "  Vdata (Mb):");
  }
  return (uint64_t)t[0];
}

uint64_t MapReduce::kmv_stats(int level) {  // :2972-3001
  ensure_resident();
  need_kmv("print stats");
  const KMV& m = *kmv;
  const int64_t vb = m.vw >= 0 ? m.nval * m.vw : (m.nval ? m.voff[m.nval].item<int64_t>() : 0);
  std::vector<int64_t> t = comm_->allreduce({m.nkey, m.keys.key_bytes(), vb, m.nbytes(), pages(m.nbytes())}, Comm::SUM);
  const double mb = 1024.0 * 1024.0;
  if (level == 1 && comm_->rank() == 0)
    out(fmt("%" PRId64 " pairs, %.3g Mb keys, %.3g Mb values, %.3g Mb, %" PRId64 " pages\n", t[0], t[1] / mb,
            t[2] / mb, t[3] / mb, t[4]));
  if (level == 2) {
    histo((double)m.nkey, "  KMV pairs:");
    histo(m.keys.key_bytes() / mb, "  Kdata (Mb):");
    histo(vb / mb, "  Vdata (Mb):");
  }
  return (uint64_t)t[0];
}

void MapReduce::cummulative_stats(int level, int reset) {  // :3007-3066
  const double mb = 1024.0 * 1024.0, gb = mb * 1024.0;
  const int me = comm_->rank();
  if (me == 0) out("MapReduce-MPI (gpu_mapreduce_amd native engine)\n");
  int64_t mx = comm_->allreduce(msizemax.load(), Comm::MAX), sm = comm_->allreduce(msizemax.load(), Comm::SUM);
  if (me == 0) out(fmt("Cummulative hi-water mem = %.3g Mb any proc, %.3g Gb all procs\n", mx / mb, sm / gb));
  std::vector<int64_t> c = comm_->allreduce({cssize.load(), crsize.load()}, Comm::SUM);
  double ct = comm_->allreduce_f64(commtime, Comm::SUM);
  if (c[0] || c[1]) {
    if (me == 0)
      out(fmt("Cummulative comm = %.3g Mb send, %.3g Mb recv, %.3g secs\n", c[0] / mb, c[1] / mb,
              ct / comm_->size()));
    if (level == 2) {
      histo(cssize / mb, "  Send (Mb):");
      histo(crsize / mb, "  Recv (Mb):");
    }
  }
  std::vector<int64_t> io = comm_->allreduce({rsize.load(), wsize.load()}, Comm::SUM);
  if ((io[0] || io[1]) && me == 0) out(fmt("Cummulative I/O = %.3g Mb read, %.3g Mb write\n", io[0] / mb, io[1] / mb));
  if (hbm::installed() && device().is_cuda()) {  // the page pool's hi-water mark (reference hiwater())
    const hbm::PoolStats ps = hbm::stats(device().index() < 0 ? 0 : device().index());
    const int64_t hp = comm_->allreduce(ps.peak, Comm::MAX);
    if (me == 0)
      out(fmt("HBM page pool: hi-water %.3g Mb any proc, %.3g Mb in use, %.3g Mb reserved, %lld failed requests\n",
              hp / mb, ps.in_use / mb, ps.reserved / mb, (long long)ps.failures));
  }
  if (reset) rsize = wsize = cssize = crsize = 0;
}

// ====================================================================== spill tier

void MapReduce::spill() {
  flatten();
  flatten_kmv();
  const bool pin = device().is_cuda();
  if (kv) kv = kv_host(*kv, pin);
  if (kmv) kmv = kmv_to(*kmv, at::Device(at::kCPU), pin);
}

void MapReduce::unspill() {
  flatten_kmv();
  if (kv) kv = kv_to(*kv, device());
  if (kmv) kmv = kmv_to(*kmv, device(), false);
}

}  // namespace mrh

// ====================================================================== checkpoint

namespace mrh {

namespace {
constexpr char kMagic[8] = {'M', 'R', 'H', 'K', 'V', '0', '0', '1'};

std::string rank_path(const std::string& p, const Comm& c) {
  return c.size() > 1 ? p + "." + std::to_string(c.rank()) : p;
}
void put_i64(std::FILE* f, int64_t v) {
  if (std::fwrite(&v, 8, 1, f) != 1) throw std::runtime_error("save: write failed");
}
int64_t get_i64(std::FILE* f) {
  int64_t v = 0;
  if (std::fread(&v, 8, 1, f) != 1) throw std::runtime_error("load: truncated file");
  return v;
}
// tensor as (present, dtype, numel, bytes)
void put_t(std::FILE* f, const at::Tensor& t) {
  put_i64(f, t.defined() ? 1 : 0);
  if (!t.defined()) return;
  at::Tensor h = t.to(at::kCPU).contiguous();
  put_i64(f, (int64_t)h.scalar_type());
  put_i64(f, h.numel());
  const size_t nb = (size_t)h.numel() * h.element_size();
  if (nb && std::fwrite(h.data_ptr(), 1, nb, f) != nb) throw std::runtime_error("save: write failed");
}
at::Tensor get_t(std::FILE* f, at::Device dev) {
  const int64_t present = get_i64(f);
  if (present == 0) return at::Tensor();
  if (present != 1) throw std::runtime_error("load: corrupt tensor header");
  const int64_t code = get_i64(f);
  // only the dtypes a KV/KMV column can have (byte arenas, int32/int64 offsets)
  if (code != (int64_t)at::kByte && code != (int64_t)at::kInt && code != (int64_t)at::kLong)
    throw std::runtime_error("load: unexpected tensor dtype code " + std::to_string(code));
  const int64_t n = get_i64(f);
  if (n < 0 || n > (int64_t(1) << 46)) throw std::runtime_error("load: corrupt tensor length");
  at::Tensor h = at::empty({n}, at::TensorOptions().dtype((at::ScalarType)code));
  const size_t nb = (size_t)n * h.element_size();
  if (nb && std::fread(h.data_ptr(), 1, nb, f) != nb) throw std::runtime_error("load: truncated file");
  return h.to(dev);
}
void put_kv(std::FILE* f, const KV& kv) {
  put_i64(f, kv.n);
  put_i64(f, kv.kw);
  put_i64(f, kv.vw);
  put_t(f, kv.kdata);
  put_t(f, kv.koff);
  put_t(f, kv.vdata);
  put_t(f, kv.voff);
}
KV get_kv(std::FILE* f, at::Device dev) {
  KV kv;
  kv.n = get_i64(f);
  const int64_t kw = get_i64(f), vw = get_i64(f);
  if (kv.n < 0 || kw < -1 || vw < -1 || kw > (1 << 30) || vw > (1 << 30))
    throw std::runtime_error("load: corrupt KV header");
  kv.kw = (int)kw;
  kv.vw = (int)vw;
  kv.kdata = get_t(f, dev);
  kv.koff = get_t(f, dev);
  kv.vdata = get_t(f, dev);
  kv.voff = get_t(f, dev);
  return kv;
}
}  // namespace

void MapReduce::save(const std::string& path) const {
  if (disk_path_.empty() && !kv && !kmv) fail("Cannot save without KeyValue or KeyMultiValue");
  const_cast<MapReduce*>(this)->ensure_resident();
  const_cast<MapReduce*>(this)->flatten();
  const_cast<MapReduce*>(this)->flatten_kmv();
  write_file(rank_path(path, *comm_));
}

namespace {
struct FileCloser {
  void operator()(std::FILE* f) const {
    if (f) std::fclose(f);
  }
};
using FilePtr = std::unique_ptr<std::FILE, FileCloser>;
}  // namespace

void MapReduce::write_file(const std::string& p) const {
  FilePtr f(std::fopen(p.c_str(), "wb"));
  if (!f) fail("Could not open checkpoint file " + p);
  try {
    if (std::fwrite(kMagic, 1, 8, f.get()) != 8) throw std::runtime_error("save: write failed");
    if (kv) {
      put_i64(f.get(), 0);
      put_kv(f.get(), *kv);
    } else {
      put_i64(f.get(), 1);
      put_kv(f.get(), kmv->keys);
      put_i64(f.get(), kmv->nkey);
      put_i64(f.get(), kmv->nval);
      put_i64(f.get(), kmv->vw);
      put_t(f.get(), kmv->vdata);
      put_t(f.get(), kmv->voff);
      put_t(f.get(), kmv->seg);
    }
    const long bytes = std::ftell(f.get());
    // a full disk shows up at the final flush: never leave a truncated file that looks valid
    if (std::fclose(f.release()) != 0) throw std::runtime_error("save: close failed (disk full?)");
    wsize += bytes;
  } catch (...) {
    f.reset();
    std::remove(p.c_str());
    throw;
  }
}

uint64_t MapReduce::load(const std::string& path) {
  drop_disk();
  return count(read_file(rank_path(path, *comm_)));
}

int64_t MapReduce::read_file(const std::string& p) {
  FilePtr f(std::fopen(p.c_str(), "rb"));
  if (!f) fail("Could not open checkpoint file " + p);
  char magic[8];
  if (std::fread(magic, 1, 8, f.get()) != 8 || std::memcmp(magic, kMagic, 8) != 0)
    fail("Not a gpu_mapreduce_amd checkpoint: " + p);
  int64_t n = 0;
  const int64_t kind = get_i64(f.get());
  if (kind == 0) {
    KV k = get_kv(f.get(), device());
    guard::check_kv(k, "load");  // offsets/arena sizes consistent before any kernel reads them
    kv = k;
    kv_tail_.clear();
    drop_kmv();
    n = kv->n;
  } else if (kind == 1) {
    KMV m;
    m.keys = get_kv(f.get(), device());
    m.nkey = get_i64(f.get());
    m.nval = get_i64(f.get());
    const int64_t vw = get_i64(f.get());
    if (m.nkey < 0 || m.nval < 0 || vw < -1 || vw > (1 << 30)) throw std::runtime_error("load: corrupt KMV header");
    m.vw = (int)vw;
    m.vdata = get_t(f.get(), device());
    m.voff = get_t(f.get(), device());
    m.seg = get_t(f.get(), device());
    guard::check_kmv(m, "load");
    kmv = m;
    kv.reset();
    kv_tail_.clear();
    n = m.nkey;
  } else {
    fail("load: corrupt checkpoint kind in " + p);
  }
  rsize += std::ftell(f.get());
  return n;
}

// ---------------------------------------------------------------- disk tier
// The third memory tier (HBM -> pinned host -> disk): the data goes to a
// per-rank file named like the reference's out-of-core files
// (fpath/mrmpi.<kv|kmv>.<instance>.<counter>.<rank>, src/mapreduce.cpp:3187-3205)
// and comes back on the MR's next op (ensure_resident, called from the op frame's enter()).
void MapReduce::spill_disk() {
  flatten();
  flatten_kmv();
  if (!kv && !kmv) return;
  char name[96];
  std::snprintf(name, sizeof(name), "mrmpi.%s.%d.%d.%d", kv ? "kv" : "kmv", instance_me_, ++disk_counter_,
                comm_->rank());
  const std::string p = (std::filesystem::path(set.fpath) / name).string();
  write_file(p);
  kv.reset();
  drop_kmv();
  disk_path_ = p;
}

void MapReduce::ensure_resident() {
  if (disk_path_.empty()) return;
  const std::string p = disk_path_;
  disk_path_.clear();
  read_file(p);
  std::remove(p.c_str());
}

void MapReduce::drop_for_map(int addflag, const MapReduce* src) {
  // the reference deletes kv/kmv at the start of a map too (src/mapreduce.cpp:1044-1051)
  if (addflag || src == this) return;
  drop_disk();
  kv.reset();
  kv_tail_.clear();
  drop_kmv();
  grouped_.reset();
}

void MapReduce::drop_disk() {
  if (disk_path_.empty()) return;
  std::remove(disk_path_.c_str());
  disk_path_.clear();
}

}  // namespace mrh
