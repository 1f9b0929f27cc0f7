// Device functors (devfn.h), the host side: user device code compiled at run
// time by hiprtc for gfx950 around the device text of devfn_text.cpp. A map /
// reduce functor becomes two kernels —
//
//   mrd_count  one thread per item (pair / task / key, grid-stride): runs the
//              functor with a counting Emit, stores the item's records, key
//              bytes and value bytes, and min/max record widths (atomics)
//   mrd_write  runs it again with a writing Emit at the item's offsets (the
//              exclusive scans of the counts) into var-width output columns
//
// A uniform output width (every key, every value the same length) turns
// into a fixed-width KV, so later ops keep their fixed-key fast paths.
// The other kinds have kernels of their own (the kind table below). Every
// kernel that runs user code takes the bound buffers (devfn.h Args) as its
// last argument, by value. Modules are cached per (device, kind, scan shape,
// code).
#include "devfn.h"

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <unordered_map>
#include <vector>

#include "../kernels/launch.h"
#include "devfn_text.h"

namespace mrh {
namespace devfn {

// the by-value ABI: mrd::Args / mrd::MutArgs in the prelude assert the same
// size and offset against MRD_ARGS_BYTES, which source_of defines from here
static_assert(sizeof(Args::Buf) == 16 && sizeof(Args) == kMaxArgs * 16 + 8 && offsetof(Args, n) == kMaxArgs * 16,
              "devfn::Args is kMaxArgs x {pointer, bytes} and a count: the layout the functor kernels take");

namespace {
// rows per workgroup tile of the comparator sort (256 threads, 8 rows each)
constexpr int64_t kCompareTile = 2048;
// the LDS stage of mrd_text_write. A tile is 256 items; at the 60 - 130 bytes
// a line of an index or a table takes, 256 lines are 15 - 33 KiB, so 32 KiB
// stages nearly every such tile and still leaves room for four workgroups
// (16 waves) on a CU's 160 KiB
constexpr int64_t kTextStage = 32768;

// a kind's entry points, in the order of its table row
enum EmitFn { kCount, kWrite, kAccSize, kFoldNChunks, kFoldChunks, kFoldMerge };  // Map, Reduce: the first two
enum SortKeyFn { kSortKey };
enum CompareFn { kBlockSort, kMerge };
enum ScanFn { kScan };
enum HashFn { kHash };
enum PrintFn { kTextCount, kTextWrite };
constexpr int kMaxEntries = 6;

struct KindRow {
  const char* file;                  // the source's name in compiler logs
  const char* define;                // defined in front of the prelude (null: nothing) ...
  int64_t value;                     // ... as this value; Scan, Print: plus the shape (0 KV, 1 KMV)
  const char* kernels;               // the device text after the user's code
  const char* entries[kMaxEntries];  // the kernels to resolve
  const char* whose;                 // for the load error
};
// Kernel parameters, for the launches below (i64 = int64_t; col = const u8* d,
// const i64* off, i64 w; items = col k, col v, const i64* seg):
//   mrd_count         (items, i64 first, i64 n, i64* cnt, u64* wid, int bytes, Args)
//   mrd_write         (items, i64 first, i64 n, const i64* pr, const i64* pk, const i64* pv, i64 okw, i64 ovw,
//                      u8* okd, i64* okoff, u8* ovd, i64* ovoff, Args)
//   mrd_acc_size      (i64* out)
//   mrd_fold_nchunks  (const i64* seg, i64 nkey, i64 C, i64* cnt, u64* maxc)
//   mrd_fold_chunks   (items, i64 nkey, const i64* cstart, i64 nchunk, i64 C, u8* accs, Args)
//   mrd_fold_merge    (const i64* cstart, i64 nkey, i64 nchunk, i64 stride, u8* accs, Args)
//   mrd_sortkey       (col, i64 n, u64* key, u32* idx, Args)
//   mrd_cmp_blocksort (col, const i64* sid, i64 n, u32* out, Args)
//   mrd_cmp_merge     (col, const i64* sid, i64 n, const u32* src, u32* dst, i64 W, Args)
//   mrd_scan          (items, i64 base, i64 n, MutArgs)
//   mrd_hash          (col, i64 n, int P, int* dest, Args)
//   mrd_text_count    (items, i64 base, i64 n, i64* cnt, Args)
//   mrd_text_write    (items, i64 base, i64 n, const i64* pre, u8* out, int stage_ok, u64* tiles, Args)
// MapText has mrd_count / mrd_write of its own: the same parameters with
//   records = const u8* text, const i64* off, i64 trim, i64 file, i64 base
// in the place of items
const KindRow kKinds[] = {
    {"mrd_map.hip", "MRD_REDUCE", 0, text::kEmitKernels, {"mrd_count", "mrd_write"}, "the device functor's"},
    {"mrd_reduce.hip", "MRD_REDUCE", 1, text::kEmitKernels, {"mrd_count", "mrd_write"}, "the device functor's"},
    {"mrd_fold.hip", "MRD_REDUCE", 2, text::kEmitKernels,
     {"mrd_count", "mrd_write", "mrd_acc_size", "mrd_fold_nchunks", "mrd_fold_chunks", "mrd_fold_merge"},
     "the device functor's"},
    {"mrd_sortkey.hip", nullptr, 0, text::kSortKeyKernel, {"mrd_sortkey"}, "the sort-key functor's"},
    {"mrd_compare.hip", "MRD_CMP_T", kCompareTile, text::kCompareKernels, {"mrd_cmp_blocksort", "mrd_cmp_merge"},
     "the comparator functor's"},
    {"mrd_scan.hip", "MRD_SCAN_KMV", 0, text::kScanKernel, {"mrd_scan"}, "the scan functor's"},
    {"mrd_hash.hip", nullptr, 0, text::kHashKernel, {"mrd_hash"}, "the partitioner functor's"},
    {"mrd_map_text.hip", nullptr, 0, text::kTextKernels, {"mrd_count", "mrd_write"}, "the device functor's"},
    {"mrd_print.hip", "MRD_PRINT_KMV", 0, text::kPrintKernels, {"mrd_text_count", "mrd_text_write"},
     "the print functor's"},
};
const KindRow& row_of(Kind kind) { return kKinds[(int)kind]; }

// the full source of a functor; kmv: the KMV shape of mr_scan / mr_print (Scan, Print only)
std::string source_of(const std::string& code, Kind kind, bool kmv = false) {
  const KindRow& r = row_of(kind);
  std::string src = "#define MRD_ARGS_BYTES " + std::to_string(sizeof(Args)) + "\n";
  if (r.define) src += std::string("#define ") + r.define + " " + std::to_string(r.value + kmv) + "\n";
  if (kind == Kind::Print) src += "#define MRD_TEXT_STAGE " + std::to_string(kTextStage) + "\n";
  return src + text::kPrelude + code + "\n" + r.kernels;
}

Kind kind_of(const std::string& code, bool reduce) {
  return !reduce ? Kind::Map : code.find("mr_finish") != std::string::npos ? Kind::Fold : Kind::Reduce;
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

// compile only: the code object's size
int64_t check(const std::string& code, Kind kind, bool kmv = false) {
  return (int64_t)compile(source_of(code, kind, kmv), row_of(kind).file).size();
}

struct Module {
  hipModule_t mod = nullptr;
  hipFunction_t fn[kMaxEntries] = {};  // indexed by the kind's entry enum
};

const Module& module_for(const std::string& code, Kind kind, int device, bool kmv = false) {
  static std::mutex mu;
  static std::unordered_map<std::string, std::unique_ptr<Module>> cache;
  const std::string key =
      std::to_string(device) + ":" + std::to_string((int)kind) + ":" + std::to_string((int)kmv) + ":" + code;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return *it->second;
  const KindRow& r = row_of(kind);
  const std::string obj = compile(source_of(code, kind, kmv), r.file);
  auto m = std::make_unique<Module>();
  bool ok = hipModuleLoadData(&m->mod, obj.data()) == hipSuccess;
  for (int i = 0; ok && i < kMaxEntries && r.entries[i]; ++i)
    ok = hipModuleGetFunction(&m->fn[i], m->mod, r.entries[i]) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    throw std::runtime_error(std::string("mrhip: loading ") + r.whose + " code object failed");
  }
  return *cache.emplace(key, std::move(m)).first->second;
}

// a partitioner source without its entry point would only fail inside the call
// shim. A heuristic (a substring search, as sort_kind_of): code that names
// mr_hash only in a comment or as part of a longer name passes it and gets the
// shim's compiler log instead
void need_hash(const std::string& code) {
  if (code.find("mr_hash") == std::string::npos)
    throw std::runtime_error(
        "mrhip: a device partitioner functor defines `int mr_hash(mrd::Bytes key)` (MR-MPI's hash callback: the "
        "pair's owner is the result mod the number of ranks); the code has no mr_hash");
}

// the same for a print source
void need_print(const std::string& code) {
  if (code.find("mr_print") == std::string::npos)
    throw std::runtime_error(
        "mrhip: a device print functor defines `void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, "
        "mrd::Text& out)` (KV) or `void mr_print(mrd::Bytes key, mrd::Values values, mrd::Text& out)` (KMV); the code "
        "has no mr_print");
}

void need_gpu(at::Device dev) {
  if (!dev.is_cuda()) throw std::runtime_error("mrhip: device functors run on a GPU MapReduce (device cuda)");
}

template <typename T>
T* P0(const at::Tensor& t) {
  return t.defined() && t.numel() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}
at::TensorOptions opt(at::Device d, at::ScalarType t) { return at::TensorOptions().device(d).dtype(t); }

// The one launch: 256 threads a workgroup, the arguments in kernel order. The
// runtime gets a pointer to every argument and copies as many bytes from it as
// the kernel's parameter has, so the pack's types must be the kernel's
// parameter types exactly (the lists above the kind table): convert at the
// call site, nothing is promoted here.
template <class... Ts>
void launch(hipFunction_t f, unsigned grid, hipStream_t s, const Ts&... a) {
  void* ptrs[] = {const_cast<void*>(static_cast<const void*>(&a))...};
  if (hipModuleLaunchKernel(f, grid, 1, 1, 256, 1, 1, 0, s, ptrs, nullptr) != hipSuccess) {
    (void)hipGetLastError();
    throw std::runtime_error("mrhip: device functor launch failed");
  }
}
// the grid of a grid-stride kernel over n items
unsigned grid_of(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 65536)); }

// one column as the kernels take it: fixed width w (off null) or offsets (w 0)
struct Column {
  const uint8_t* d = nullptr;
  const int64_t* off = nullptr;
  int64_t w = 0;
};
Column column_of(const at::Tensor& data, const at::Tensor& off, int w) {
  return {P0<uint8_t>(data), w >= 0 ? nullptr : P0<int64_t>(off), w >= 0 ? w : 0};
}
// the items of a launch: n pairs from `first` on (seg null; no columns: tasks) or n keys with their values
struct Items {
  Column k, v;
  const int64_t* seg = nullptr;
  int64_t first = 0, n = 0;
};
Items items_of(const KV& kv, int64_t first, int64_t n) {
  return {column_of(kv.kdata, kv.koff, kv.kw), column_of(kv.vdata, kv.voff, kv.vw), nullptr, first, n};
}
Items items_of(const KMV& m) {
  return {column_of(m.keys.kdata, m.keys.koff, m.keys.kw), column_of(m.vdata, m.voff, m.vw), P0<int64_t>(m.seg), 0,
          m.nkey};
}
// a grid-stride kernel over `threads` whose parameters start with the items' columns
template <class... Ts>
void launch_items(hipFunction_t f, int64_t threads, hipStream_t s, const Items& it, const Ts&... rest) {
  launch(f, grid_of(threads), s, it.k.d, it.k.off, it.k.w, it.v.d, it.v.off, it.v.w, it.seg, rest...);
}

// The two-pass emit over `n` items from `first` on: head(f, rest...) launches
// kernel f over them with the kind's leading parameters (its items) in front
// of rest
template <class Head>
KV run_emit(int64_t first, int64_t n, const Head& head, const std::string& code, Kind kind, at::Device dev,
            const Args& bound) {
  struct {
    int64_t first, n;
  } it{first, n};
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
    head(m.fn[kCount], it.first, it.n, P0<int64_t>(cnt), P0<int64_t>(wid), bytes, bound);
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
  if (nout)
    head(m.fn[kWrite], it.first, it.n, P0<int64_t>(pr), P0<int64_t>(pk), P0<int64_t>(pv), okw, ovw,
         P0<uint8_t>(out.kdata), P0<int64_t>(out.koff), P0<uint8_t>(out.vdata), P0<int64_t>(out.voff), bound);
  if (out.koff.defined()) k::fill_i64(P0<int64_t>(out.koff) + nout, 1, tot[1], s);
  if (out.voff.defined()) k::fill_i64(P0<int64_t>(out.voff) + nout, 1, tot[2], s);
  return out;
}

KV run(const Items& it, const std::string& code, Kind kind, at::Device dev, const Args& bound) {
  hipStream_t s = at::hip::getCurrentHIPStream();
  return run_emit(
      it.first, it.n, [&](hipFunction_t f, const auto&... rest) { launch_items(f, it.n, s, it, rest...); }, code, kind,
      dev, bound);
}

// fold tier: accumulators per chunk of values, merged per key, then mr_finish per key
KV run_fold(const Items& it, const std::string& code, at::Device dev, const Args& bound) {
  if (!it.n) return run(it, code, Kind::Fold, dev, bound);
  const Module& mod = module_for(code, Kind::Fold, dev.index());
  hipStream_t s = at::hip::getCurrentHIPStream();
  static const int64_t C = [] {
    const char* e = std::getenv("MRH_FOLD_CHUNK");
    return e && std::atoll(e) > 0 ? std::atoll(e) : int64_t(256);
  }();
  at::Tensor asz_t = at::empty({1}, opt(dev, at::kLong));
  launch(mod.fn[kAccSize], 1u, s, P0<int64_t>(asz_t));
  at::Tensor cnt = at::empty({it.n + 1}, opt(dev, at::kLong));  // + the most chunks of one key
  if (hipMemsetAsync(P0<int64_t>(cnt) + it.n, 0, 8, s) != hipSuccess)
    throw std::runtime_error("mrhip: hipMemsetAsync failed");
  launch(mod.fn[kFoldNChunks], grid_of(it.n), s, it.seg, it.n, C, P0<int64_t>(cnt), P0<int64_t>(cnt) + it.n);
  at::Tensor cstart = exclusive_scan(cnt.narrow(0, 0, it.n));
  int64_t asz = 0, nchunk = 0, maxc = 0;
  read_small(s, {{P0<int64_t>(asz_t), &asz, 8}, {P0<int64_t>(cstart) + it.n, &nchunk, 8},
                 {P0<int64_t>(cnt) + it.n, &maxc, 8}});
  at::Tensor accs = at::empty({std::max<int64_t>(1, nchunk * asz)}, opt(dev, at::kByte));
  launch_items(mod.fn[kFoldChunks], nchunk, s, it, it.n, P0<int64_t>(cstart), nchunk, C, P0<uint8_t>(accs), bound);
  for (int64_t stride = 1; stride < maxc; stride *= 2)
    launch(mod.fn[kFoldMerge], grid_of(nchunk), s, P0<int64_t>(cstart), it.n, nchunk, stride, P0<uint8_t>(accs),
           bound);
  Items f = it;  // mr_finish reads the merged accumulators where the values were
  f.v = {P0<uint8_t>(accs), P0<int64_t>(cstart), asz};
  f.seg = nullptr;
  return run(f, code, Kind::Fold, dev, bound);
}

int64_t run_scan(const Items& it, const std::string& code, bool kmv, at::Device dev, const Args& bound) {
  if (it.n <= 0) return 0;
  const Module& m = module_for(code, Kind::Scan, dev.index(), kmv);
  launch_items(m.fn[kScan], it.n, at::hip::getCurrentHIPStream(), it, it.first, it.n, bound);
  return it.n;
}

// the write kernel's tile counters, {staged, direct}: two u64 of device memory
// per device that ran a print functor, kept for the life of the process
std::mutex g_tiles_mu;
std::unordered_map<int, unsigned long long*> g_tiles;
unsigned long long* tiles_of(int device, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_tiles_mu);
  auto it = g_tiles.find(device);
  if (it != g_tiles.end()) return it->second;
  unsigned long long* p = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&p), 16) != hipSuccess || hipMemsetAsync(p, 0, 16, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    (void)hipGetLastError();
    throw std::runtime_error("mrhip: allocating the print functor's tile counters failed");
  }
  return g_tiles.emplace(device, p).first->second;
}
int64_t env_i64(const char* name, int64_t dflt) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoll(e) : dflt;
}

// count, scan, write: the text of the items, one contiguous range in item order
at::Tensor run_print(const Items& it, const std::string& code, bool kmv, at::Device dev, const Args& bound) {
  need_print(code);
  if (it.n <= 0) return at::empty({0}, opt(dev, at::kByte));
  const Module& m = module_for(code, Kind::Print, dev.index(), kmv);
  hipStream_t s = at::hip::getCurrentHIPStream();
  at::Tensor cnt = at::empty({it.n}, opt(dev, at::kLong));
  launch_items(m.fn[kTextCount], it.n, s, it, it.first, it.n, P0<int64_t>(cnt), bound);
  at::Tensor pre = exclusive_scan(cnt);
  int64_t bytes = 0;
  read_small(s, {{P0<int64_t>(pre) + it.n, &bytes, 8}});
  // MRH_TEXT_LEAD (debug): the text starts that many bytes (mod 16) into its
  // allocation, as the text of a later piece does inside a larger buffer;
  // MRH_TEXT_STAGE=0 (measurements): every tile takes the direct route
  const int64_t lead = env_i64("MRH_TEXT_LEAD", 0) & 15;
  const int stage_ok = env_i64("MRH_TEXT_STAGE", 1) != 0;
  at::Tensor out = at::empty({bytes + lead}, opt(dev, at::kByte)).narrow(0, lead, bytes);
  if (!bytes) return out;
  const int64_t ntile = (it.n + 255) / 256;
  const Items& i = it;
  launch(m.fn[kTextWrite], (unsigned)std::min<int64_t>(ntile, 65536), s, i.k.d, i.k.off, i.k.w, i.v.d, i.v.off, i.v.w,
         i.seg, i.first, i.n, (const int64_t*)P0<int64_t>(pre), P0<uint8_t>(out), stage_ok,
         tiles_of(dev.index() < 0 ? 0 : dev.index(), s), bound);
  return out;
}
}  // namespace

std::string full_source(const std::string& code, bool reduce) { return source_of(code, kind_of(code, reduce)); }

int64_t compile_check(const std::string& code, bool reduce) { return check(code, kind_of(code, reduce)); }
int64_t compile_check_text(const std::string& code) { return check(code, Kind::MapText); }
int64_t compile_check_sortkey(const std::string& code) { return check(code, Kind::SortKey); }
int64_t compile_check_compare(const std::string& code) { return check(code, Kind::Compare); }
int64_t compile_check_scan(const std::string& code, bool kmv) { return check(code, Kind::Scan, kmv); }
int64_t compile_check_hash(const std::string& code) {
  need_hash(code);
  return check(code, Kind::Hash);
}
int64_t compile_check_print(const std::string& code, bool kmv) {
  need_print(code);
  return check(code, Kind::Print, kmv);
}
int64_t text_stage_bytes() { return kTextStage; }
std::pair<int64_t, int64_t> text_tiles() {
  std::lock_guard<std::mutex> lk(g_tiles_mu);
  std::pair<int64_t, int64_t> t{0, 0};
  int cur = 0;
  if (!g_tiles.empty() && hipGetDevice(&cur) != hipSuccess) throw std::runtime_error("mrhip: hipGetDevice failed");
  for (const auto& e : g_tiles) {
    unsigned long long c[2] = {0, 0};
    const bool ok = hipSetDevice(e.first) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(c, e.second, 16, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipSetDevice(cur);
    if (!ok) {
      (void)hipGetLastError();
      throw std::runtime_error("mrhip: reading the print functor's tile counters failed");
    }
    t.first += (int64_t)c[0];
    t.second += (int64_t)c[1];
  }
  return t;
}
int64_t compile_count() { return g_compiles.load(); }
int64_t compare_tile() { return kCompareTile; }

Kind sort_kind_of(const std::string& code) {
  if (code.find("mr_sortkey") != std::string::npos) return Kind::SortKey;
  if (code.find("mr_compare") != std::string::npos) return Kind::Compare;
  throw std::runtime_error(
      "mrhip: a device sort functor defines `unsigned long long mr_sortkey(mrd::Bytes)` (radix sort by a 64-bit key) "
      "or `int mr_compare(mrd::Bytes, mrd::Bytes)` (merge sort by a comparator); the code has neither");
}

Args args_of(const std::vector<at::Tensor>& bufs) {
  if ((int)bufs.size() > kMaxArgs)
    throw std::runtime_error("mrhip: a device functor takes at most " + std::to_string(kMaxArgs) + " bound buffers, " +
                             std::to_string(bufs.size()) + " given");
  Args g{};
  g.n = (int)bufs.size();
  for (int i = 0; i < g.n; ++i) g.a[i] = {bufs[i].numel() ? bufs[i].data_ptr() : nullptr, (int64_t)bufs[i].nbytes()};
  return g;
}

KV map_pairs(const KV& kv_in, const std::string& code, at::Device dev, int64_t a, int64_t b, const Args& bound) {
  need_gpu(dev);
  KV kv = kv_in.device() == dev ? kv_in : kv_to(kv_in, dev);
  if (b < 0 || b > kv.n) b = kv.n;
  return run(items_of(kv, a, std::max<int64_t>(0, b - a)), code, Kind::Map, dev, bound);
}

KV map_tasks(int64_t first, int64_t n, const std::string& code, at::Device dev, const Args& bound) {
  need_gpu(dev);
  Items it;
  it.first = first;
  it.n = n;
  return run(it, code, Kind::Map, dev, bound);
}

KV map_records(const at::Tensor& text, const at::Tensor& off, int64_t nrec, int64_t trim, int64_t file, int64_t base,
               const std::string& code, at::Device dev, int64_t a, int64_t b, const Args& bound) {
  need_gpu(dev);
  if (b < 0 || b > nrec) b = nrec;
  a = std::max<int64_t>(a, 0);
  if (b > a && (!text.is_cuda() || !off.is_cuda() || off.numel() < nrec + 1))
    throw std::runtime_error("mrhip: map_records needs the text and its nrec + 1 record offsets in HBM");
  hipStream_t s = at::hip::getCurrentHIPStream();
  const uint8_t* t = P0<uint8_t>(text);
  const int64_t* o = P0<int64_t>(off);
  return run_emit(
      a, b - a,
      [&](hipFunction_t f, const auto&... rest) { launch(f, grid_of(b - a), s, t, o, trim, file, base, rest...); }, code,
      Kind::MapText, dev, bound);
}

KV reduce_groups(const KMV& m, const std::string& code, at::Device dev, const Args& bound) {
  if (m.nkey && !m.seg.is_cuda()) throw std::runtime_error("mrhip: reduce_device needs the groups in HBM");
  need_gpu(dev);
  if (kind_of(code, true) == Kind::Reduce) return run(items_of(m), code, Kind::Reduce, dev, bound);
  return run_fold(items_of(m), code, dev, bound);
}

std::pair<at::Tensor, at::Tensor> sort_keys_of(const at::Tensor& data, const at::Tensor& off, int w, int64_t n,
                                               const std::string& code, at::Device dev, const Args& bound) {
  need_gpu(dev);
  at::Tensor key = at::empty({std::max<int64_t>(n, 1)}, opt(dev, at::kLong));
  at::Tensor idx = at::empty({std::max<int64_t>(n, 1)}, opt(dev, at::kInt));
  if (n > 0) {
    const Module& m = module_for(code, Kind::SortKey, dev.index());
    const Column c = column_of(data, off, w);
    launch(m.fn[kSortKey], grid_of(n), at::hip::getCurrentHIPStream(), c.d, c.off, c.w, n, P0<int64_t>(key),
           P0<int32_t>(idx), bound);
  }
  return {key.narrow(0, 0, n), idx.narrow(0, 0, n)};
}

at::Tensor compare_perm(const at::Tensor& data, const at::Tensor& off, int w, int64_t n, const at::Tensor& sid,
                        const std::string& code, at::Device dev, const Args& bound) {
  need_gpu(dev);
  if (n > (int64_t)UINT32_MAX)
    throw std::runtime_error("mrhip: the comparator sort indexes rows with 32 bits; " + std::to_string(n) +
                             " rows are more than 4294967295");
  if (sid.defined() && sid.numel() < n) throw std::runtime_error("mrhip: compare_perm: fewer segment ids than rows");
  at::Tensor a = at::empty({std::max<int64_t>(n, 1)}, opt(dev, at::kInt));
  if (n <= 0) return a.narrow(0, 0, 0);
  at::Tensor b = n > kCompareTile ? at::empty({n}, opt(dev, at::kInt)) : at::Tensor();
  const Module& m = module_for(code, Kind::Compare, dev.index());
  hipStream_t s = at::hip::getCurrentHIPStream();
  const unsigned tiles = (unsigned)((n + kCompareTile - 1) / kCompareTile);  // one workgroup each, both kernels
  const Column c = column_of(data, off, w);
  const int64_t* sg = P0<int64_t>(sid);
  uint32_t* src = P0<uint32_t>(a);
  uint32_t* dst = P0<uint32_t>(b);
  launch(m.fn[kBlockSort], tiles, s, c.d, c.off, c.w, sg, n, src, bound);
  // ceil(log2(tiles)) passes, known from n alone: nothing is read back between them
  for (int64_t W = kCompareTile; W < n; W *= 2) {
    launch(m.fn[kMerge], tiles, s, c.d, c.off, c.w, sg, n, src, dst, W, bound);
    std::swap(src, dst);
    std::swap(a, b);
  }
  return a;
}

at::Tensor hash_dest(const KV& kv, int P, const std::string& code, at::Device dev, const Args& bound) {
  need_gpu(dev);
  need_hash(code);
  if (P < 1) throw std::runtime_error("mrhip: hash_dest: " + std::to_string(P) + " ranks");
  if (kv.n > 0 && kv.device() != dev) throw std::runtime_error("mrhip: hash_dest needs the keys in HBM");
  // (the module first: no pairs still means a functor that compiles)
  const Module& m = module_for(code, Kind::Hash, dev.index());
  at::Tensor dest = at::empty({std::max<int64_t>(kv.n, 0)}, opt(dev, at::kInt));
  if (kv.n <= 0) return dest;
  const Column c = column_of(kv.kdata, kv.koff, kv.kw);
  launch(m.fn[kHash], grid_of(kv.n), at::hip::getCurrentHIPStream(), c.d, c.off, c.w, kv.n, P, P0<int32_t>(dest),
         bound);
  return dest;
}

int64_t scan_pairs(const KV& kv_in, int64_t base, const std::string& code, at::Device dev, const Args& bound) {
  need_gpu(dev);
  KV kv = kv_in.device() == dev ? kv_in : kv_to(kv_in, dev);
  return run_scan(items_of(kv, base, kv.n), code, false, dev, bound);
}

int64_t scan_groups(const KMV& m, const std::string& code, at::Device dev, const Args& bound) {
  need_gpu(dev);
  if (m.nkey && !m.seg.is_cuda()) throw std::runtime_error("mrhip: scan_device needs the groups in HBM");
  return run_scan(items_of(m), code, true, dev, bound);
}

at::Tensor format_pairs(const KV& kv_in, int64_t base, const std::string& code, at::Device dev, const Args& bound) {
  need_gpu(dev);
  KV kv = kv_in.device() == dev ? kv_in : kv_to(kv_in, dev);
  return run_print(items_of(kv, base, kv.n), code, false, dev, bound);
}

void load_print(const std::string& code, bool kmv, at::Device dev) {
  need_gpu(dev);
  need_print(code);
  module_for(code, Kind::Print, dev.index(), kmv);
}

at::Tensor format_groups(const KMV& m, const std::string& code, at::Device dev, const Args& bound) {
  need_gpu(dev);
  if (m.nkey && !m.seg.is_cuda()) throw std::runtime_error("mrhip: print_device needs the groups in HBM");
  return run_print(items_of(m), code, true, dev, bound);
}

}  // namespace devfn
}  // namespace mrh
