// Device functors: the engine's first callback tier (callbacks
// tier 1) — user map / reduce functions written as HIP device code, compiled
// at run time for the GPU (hiprtc, gfx950) into the engine's two-pass emit
// kernels and run over device-resident KV / KMV columns. No ATen tensor
// program and no host round trip: one thread per pair (map) or per key
// (reduce), the emitted records sized by a count pass, placed by exclusive
// scans and written by a second pass (devfn.cpp; the device text is
// devfn_text.cpp).
//
// User code defines one of
//   __device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Emit& out);
//   __device__ void mr_reduce(mrd::Bytes key, mrd::Values values, mrd::Emit& out);
// and emits with out.emit(kptr, kbytes, vptr, vbytes) or out.emit(k, v) for
// trivially copyable k, v. It must be a pure function of its arguments (it
// runs twice: count, then write). The prelude (text::kPrelude in
// devfn_text.cpp) documents mrd::Bytes / mrd::Values / mrd::Emit.
//
// The user argument (MR-MPI's `ptr`): up to kMaxArgs device buffers bound to
// the MapReduce object (set_device_args) reach every functor kernel as ONE
// by-value kernel argument, a struct of 8 x {pointer, byte count} and a count
// (Args below = mrd::Args in the prelude; both sides assert the layout). No
// global symbol in the module, no allocation, nothing shared between two ops
// that run one cached module; the module cache key stays (device, kind, scan
// shape, code), so new contents or new buffers never recompile. Every entry
// point (mr_map, mr_reduce, mr_init, mr_add, mr_merge, mr_finish, mr_sortkey,
// mr_compare, mr_hash, mr_print) MAY take one trailing
// `const mrd::Args& args` parameter, each function on its own; args[i] is
// {p, n bytes} ({nullptr, 0} past the bound count), args[i].as<T>() a
// `const T*`, args[i].count<T>() the number of T. These functors run more than
// once per item (count, write) or in an unspecified order (fold, sorts): the
// buffers are read-only to them, and the purity rule now reads "a pure
// function of its arguments and the bound buffers' contents".
//
// scan (Kind::Scan) is the one functor that writes to the bound buffers:
//   __device__ void mr_scan(mrd::Bytes key, mrd::Bytes value, long long index, const mrd::MutArgs& args);  // KV
//   __device__ void mr_scan(mrd::Bytes key, mrd::Values values, const mrd::MutArgs& args);                 // KMV
// runs exactly once per item (one thread each) and emits nothing; it writes
// through args[i].as<T>() (a `T*`) with atomics or plain stores to distinct
// slots. The engine orders nothing beyond the stream.
//
// Lifetime and streams: the caller of the functions below keeps the buffers
// alive (the MapReduce object holds the bound tensors); the kernels run on the
// current stream and the buffers must be ready on it.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "kv.h"

namespace mrh {
namespace devfn {
// the functor kinds: mr_map; mr_reduce per key; the fold form (mr_init / mr_add
// / mr_merge / mr_finish); mr_sortkey; mr_compare; mr_scan; mr_hash; mr_map
// over the records of a text; mr_print
enum class Kind { Map, Reduce, Fold, SortKey, Compare, Scan, Hash, MapText, Print };
// the bound buffers as every functor kernel takes them (layout of mrd::Args /
// mrd::MutArgs in the prelude); slots past n are {nullptr, 0}
constexpr int kMaxArgs = 8;
struct Args {
  struct Buf {
    const void* p;
    int64_t n;  // bytes
  } a[kMaxArgs];
  int n;
};
// of tensors that are defined, contiguous and on one device (the caller's
// check: MapReduce::set_device_args); at most kMaxArgs
Args args_of(const std::vector<at::Tensor>& bufs);
// map: pairs [a, b) of kv (b < 0: to the end; on the GPU) through mr_map;
// index = the pair's index in kv
KV map_pairs(const KV& kv, const std::string& code, at::Device dev, int64_t a = 0, int64_t b = -1,
             const Args& args = Args{});
// map over n tasks (no input): mr_map(empty, empty, task, out)
KV map_tasks(int64_t first, int64_t n, const std::string& code, at::Device dev, const Args& args = Args{});
// map over file records: the same mr_map over records [a, b) (b < 0: to the
// end) of a text in HBM as split_records (kv.h) cut it: record i is
// text[off[i], off[i + 1] - trim), read in place. key = 8 bytes, `file` (a
// long long: the file's index in the expanded file list); value = the record;
// index = base + off[i], the byte offset of the record's first byte in its
// file when base is the file offset of text[0]. A kind of its own
// (Kind::MapText): a new text, separator or split never recompiles.
KV map_records(const at::Tensor& text, const at::Tensor& off, int64_t nrec, int64_t trim, int64_t file, int64_t base,
               const std::string& code, at::Device dev, int64_t a = 0, int64_t b = -1, const Args& args = Args{});
// compile only, as the record map compiles it; the code object size in bytes
int64_t compile_check_text(const std::string& code);
// reduce: every key of m through mr_reduce
KV reduce_groups(const KMV& m, const std::string& code, at::Device dev, const Args& args = Args{});
// compile only (syntax / type errors come back with the compiler log);
// returns the code object size in bytes. Works without a GPU.
int64_t compile_check(const std::string& code, bool reduce);
// sort-key functor: `__device__ unsigned long long mr_sortkey(mrd::Bytes b)`
// maps each key (or value) to a 64-bit key whose unsigned order is the wanted
// order (a comparator expressed as a key extraction); returns (keys [n],
// row index [n] int32) for the engine's stable radix sort
std::pair<at::Tensor, at::Tensor> sort_keys_of(const at::Tensor& data, const at::Tensor& off, int w, int64_t n,
                                               const std::string& code, at::Device dev, const Args& args = Args{});
int64_t compile_check_sortkey(const std::string& code);
// comparator functor: `__device__ int mr_compare(mrd::Bytes a, mrd::Bytes b)`
// with MR-MPI's contract (< 0 a before b, 0 equal, > 0 b before a), a strict
// weak order and a pure function of its arguments: for orders that do not fit
// a 64-bit key. Returns the stable sorted row permutation [n] int32 (u32 row
// numbers) of a merge sort that runs in the functor's compiled module. sid
// (int64 [n], may be undefined) is compared before mr_compare: rows grouped
// by segment are sorted inside every segment by one call.
at::Tensor compare_perm(const at::Tensor& data, const at::Tensor& off, int w, int64_t n, const at::Tensor& sid,
                        const std::string& code, at::Device dev, const Args& args = Args{});
// compile only; the code object size in bytes. Works without a GPU.
int64_t compile_check_compare(const std::string& code);
// rows per workgroup tile of the comparator sort (a power of two)
int64_t compare_tile();
// which sort functor the code defines: SortKey = mr_sortkey (wins when both
// names appear), Compare = mr_compare; neither is an error that names both
Kind sort_kind_of(const std::string& code);
// scan functor (mr_scan, see above) over the pairs of kv (on the GPU; index =
// base + the pair's position in kv) / over every key of m; returns the items visited
int64_t scan_pairs(const KV& kv, int64_t base, const std::string& code, at::Device dev, const Args& args);
int64_t scan_groups(const KMV& m, const std::string& code, at::Device dev, const Args& args);
// compile only (kmv: the KMV shape of mr_scan); the code object size in bytes
int64_t compile_check_scan(const std::string& code, bool kmv);
// partitioner functor: `__device__ int mr_hash(mrd::Bytes key)`, MR-MPI's
// hash callback (int hash(char* key, int keybytes)), once per pair and a pure
// function of the key and the bound buffers' contents. Returns the owner of
// every pair of kv (on the GPU), int32 [kv.n]: ((long long)h % P + P) % P, so
// negative returns and INT_MIN land where the host route puts them. P is a
// kernel argument: a new world size never recompiles. n == 0: no launch.
at::Tensor hash_dest(const KV& kv, int P, const std::string& code, at::Device dev, const Args& args = Args{});
// compile only; the code object size in bytes. Works without a GPU. A source
// without mr_hash is an error that names it (here and in hash_dest).
int64_t compile_check_hash(const std::string& code);
// print functor: the last step of a job, its result as text, formatted on the GPU.
//   __device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out);  // KV
//   __device__ void mr_print(mrd::Bytes key, mrd::Values values, mrd::Text& out);                   // KMV
// (either may take a trailing `const mrd::Args& args`) writes an item's text
// with out.put / chr / str / dec / udec / hex / fixed (mrd::Text in the
// prelude); it may write nothing. A pure function of its arguments and the
// bound buffers: it runs twice, count then write, and the write pass never
// stores past what the count pass measured. One thread per pair / per key
// (a key with very many values is formatted by one thread, as mr_reduce).
// Returns the text of kv's pairs (on the GPU; index = base + the pair's
// position) / of m's keys, in item order: uint8 [bytes] on the device. The
// write kernel stages a workgroup tile's text in LDS and copies it out in
// 16-byte lines when the tile's text fits text_stage_bytes(), and writes
// straight to HBM otherwise (devfn_text.cpp kPrintKernels). n == 0: no launch,
// an empty tensor. A source without mr_print is an error that names it.
at::Tensor format_pairs(const KV& kv, int64_t base, const std::string& code, at::Device dev, const Args& args = Args{});
at::Tensor format_groups(const KMV& m, const std::string& code, at::Device dev, const Args& args = Args{});
// compiles and loads the functor's module (a no-op once cached): print_device
// calls it before it opens a file, so a functor that does not compile leaves none behind
void load_print(const std::string& code, bool kmv, at::Device dev);
// compile only (kmv: the KMV shape of mr_print); the code object size in bytes. Works without a GPU.
int64_t compile_check_print(const std::string& code, bool kmv);
// the LDS stage of the write kernel, in bytes: a tile whose text is longer goes the direct route
int64_t text_stage_bytes();
// workgroup tiles the write kernels of this process have run so far, {staged,
// direct} (device counters, read here: synchronises the devices that ran any)
std::pair<int64_t, int64_t> text_tiles();
// hiprtc compilations this process has done so far (checks and module loads alike)
int64_t compile_count();
// the full source handed to the compiler (prelude + code + kernels)
std::string full_source(const std::string& code, bool reduce);
}  // namespace devfn
}  // namespace mrh
