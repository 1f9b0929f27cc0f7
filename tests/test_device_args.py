"""Device functor arguments (csrc/engine/devfn.h): device buffers bound to a
MapReduce object reach every functor as a trailing `const mrd::Args&`, and
scan_device runs `mr_scan` once per item with the writable `mrd::MutArgs`.

Without a GPU: the argument forms compile (every entry point, and the mix of
with / without inside one fold), the functors of test_device_functors.py
still do, binding errors name the offending index, the `args=` keyword
restores the previous binding. On the GPU every oracle is NumPy / Python on
the host and equality is exact (integers throughout)."""
import collections
import struct

import numpy as np
import pytest
import torch

from gpu_mapreduce_amd import C

import test_device_functors as old

# ---------------------------------------------------------------------- sources

# task t -> (table[t % len] % modulus, t): table = args[0] (int64), modulus = args[1][0]
MAP_TABLE = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out, const mrd::Args& args) {
  const long long* tab = args[0].as<long long>();
  const long long m = args[1].as<long long>()[0];
  out.emit((long long)(tab[t % args[0].count<long long>()] % m), (long long)t);
}
"""

# the byte count of a buffer that is not bound
PAST = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out, const mrd::Args& args) {
  out.emit((long long)t, (long long)(args[5].n + (args[5].p ? 1 : 0) + args[-1].n));
}
"""

# per-key reduce: (sum of values + 1000) * w[key] + w[key], w = args[0] (int64 per key)
REDUCE_W = r"""
__device__ void mr_reduce(mrd::Bytes key, mrd::Values vals, mrd::Emit& out, const mrd::Args& args) {
  const long long w = args[0].as<long long>()[key.as<long long>()];
  long long s = 0;
  for (long long i = 0; i < vals.n; ++i) s += vals.get<int>(i) * w;
  out.emit(key.as<long long>(), (long long)(s + 1000 * w + w));
}
"""

# the same as a fold: the weight read in mr_init (kept in the accumulator),
# in mr_add and in mr_finish; mr_merge WITHOUT the argument (the forms mix)
FOLD_W = r"""
struct mr_acc { long long k; long long s; long long c; };
__device__ void mr_init(mrd::Bytes key, mr_acc& a, const mrd::Args& args) {
  a.k = key.as<long long>();
  a.s = 0;
  a.c = 1000 * args[0].as<long long>()[a.k];
}
__device__ void mr_add(mr_acc& a, mrd::Bytes v, const mrd::Args& args) { a.s += v.as<int>() * args[0].as<long long>()[a.k]; }
__device__ void mr_merge(mr_acc& a, const mr_acc& b) { a.s += b.s; }
__device__ void mr_finish(mrd::Bytes key, const mr_acc& a, mrd::Emit& out, const mrd::Args& args) {
  out.emit(key.as<long long>(), (long long)(a.s + a.c + args[0].as<long long>()[a.k]));
}
"""

# 1000 keys: key 0 and key 1 hold one value, key 5 holds 257 (two fold chunks
# of 256), the rest of the tasks spread over keys 6 .. 905
GEN_KEYS = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  const long long k = t < 1000 ? t : t < 1256 ? 5 : 6 + t % 900;
  out.emit(k, (int)(t % 13 + 1));
}
"""
N_KEYS_TASKS = 4000

# compress over variable-width keys: (word, sum of lengths * args[0][0])
COMPRESS_SCALE = r"""
__device__ void mr_reduce(mrd::Bytes key, mrd::Values vals, mrd::Emit& out, const mrd::Args& args) {
  long long s = 0;
  for (long long i = 0; i < vals.n; ++i) s += vals.get<int>(i);
  s *= args[0].as<long long>()[0];
  out.emit(key.p, key.n, &s, 8);
}
"""

# rows for the sorts: key = a value in [0, 64), value = the row number
GEN_ROWS = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  out.emit((long long)((t * 37 + 11) % 64), (long long)t);
}
"""
GEN_ROWS_BY_VALUE = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  out.emit((long long)t, (long long)((t * 37 + 11) % 64));
}
"""
# sort by rank[key], rank = a permutation table in args[0]
SORTKEY_RANK = r"""
__device__ unsigned long long mr_sortkey(mrd::Bytes k, const mrd::Args& args) {
  return (unsigned long long)args[0].as<long long>()[k.as<long long>()];
}
"""
COMPARE_RANK = r"""
__device__ int mr_compare(mrd::Bytes a, mrd::Bytes b, const mrd::Args& args) {
  const long long* rank = args[0].as<long long>();
  const long long x = rank[a.as<long long>()], y = rank[b.as<long long>()];
  return x < y ? -1 : x > y ? 1 : 0;
}
"""
# a KMV of 3 keys whose values are {x in [0, 64), row number}
GEN_MULTI = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  const long long v[2] = {(t * 37 + 11) % 64, t};
  const long long k = t % 3;
  out.emit(&k, 8, v, 16);
}
"""

# pairs for the scans: key = a scrambled int64, value = the task number
GEN_SCAN = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  out.emit((long long)((t * 2654435761ll) >> 5 & 0xffff), (long long)t);
}
"""
# args[0] = {count, sum of index, pairs whose value == index}, args[1] = histogram of key % 16
SCAN_KV = r"""
__device__ void mr_scan(mrd::Bytes key, mrd::Bytes value, long long index, const mrd::MutArgs& args) {
  unsigned long long* acc = args[0].as<unsigned long long>();
  atomicAdd(acc + 0, 1ull);
  atomicAdd(acc + 1, (unsigned long long)index);
  if (value.as<long long>() == index) atomicAdd(acc + 2, 1ull);
  atomicAdd(args[1].as<unsigned long long>() + key.as<long long>() % 16, 1ull);
}
"""
# args[0][0] += values.n; args[1][key] = the key's largest value (a slot per key)
SCAN_KMV = r"""
__device__ void mr_scan(mrd::Bytes key, mrd::Values values, const mrd::MutArgs& args) {
  atomicAdd(args[0].as<unsigned long long>(), (unsigned long long)values.n);
  long long m = values.get<long long>(0);
  for (long long i = 1; i < values.n; ++i) m = values.get<long long>(i) > m ? values.get<long long>(i) : m;
  args[1].as<long long>()[key.as<long long>()] = m;
}
"""
# key 0: one value; key 1: 1000 values; keys 2 .. 9: the rest
GEN_GROUPS = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  const long long k = t == 0 ? 0 : t <= 1000 ? 1 : 2 + t % 8;
  out.emit(k, (long long)((t * 7919) % 100003));
}
"""

# a map over pairs: (key, value + table[index % len])
MAP_PAIRS_TABLE = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Emit& out, const mrd::Args& args) {
  const long long x = value.as<long long>() + args[0].as<long long>()[index % args[0].count<long long>()];
  out.emit(key.as<long long>(), x);
}
"""


# ---------------------------------------------------------------------- no GPU

def test_entry_points_accept_the_trailing_args():
    assert C.device_functor_check(MAP_TABLE, False) > 0
    assert C.device_functor_check(PAST, False) > 0
    assert C.device_functor_check(REDUCE_W, True) > 0
    assert C.device_functor_check(COMPRESS_SCALE, True) > 0
    assert C.device_functor_check(FOLD_W, True) > 0  # mr_add with it, mr_merge without
    assert "#define MRD_REDUCE 2" in C.device_functor_source(FOLD_W, True)
    assert C.device_sortkey_check(SORTKEY_RANK) > 0
    assert C.device_compare_check(COMPARE_RANK) > 0
    assert C.device_functor_check(MAP_PAIRS_TABLE, False) > 0


def test_functors_without_the_argument_still_compile():
    import test_device_compare as cmp
    for code, reduce in ((old.SUM_I32, True), (old.GEN, False), (old.WORDS, False), (old.FOLD, True), (old.HOT, False)):
        assert C.device_functor_check(code, reduce) > 0
    assert C.device_sortkey_check(old.SORTKEY) > 0
    assert C.device_sortkey_check(cmp.SORTKEY12) > 0
    for code in (cmp.CMP16, cmp.CMPSTR, cmp.CMP12):
        assert C.device_compare_check(code) > 0
    for code in (GEN_KEYS, GEN_ROWS, GEN_MULTI, GEN_SCAN, GEN_GROUPS):
        assert C.device_functor_check(code, False) > 0


def test_scan_functor_compiles_in_both_shapes():
    before = C.device_functor_compiles()
    assert C.device_scan_check(SCAN_KV, False) > 0
    assert C.device_scan_check(SCAN_KMV, True) > 0
    assert C.device_functor_compiles() == before + 2
    with pytest.raises(RuntimeError, match="mr_scan"):
        C.device_scan_check(old.GEN, False)
    with pytest.raises(RuntimeError, match="does not compile"):  # the KV shape where the KMV one is asked for
        C.device_scan_check(SCAN_KV, True)


def _mr(device):
    from gpu_mapreduce_amd.parallel.comm import Comm
    from gpu_mapreduce_amd.runtime.mapreduce import MapReduce
    return MapReduce(Comm(device=device))


def test_binding_errors_name_the_index():
    mr = _mr("cpu")
    ok = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"at most 8 .* 9 given \(argument 8"):
        mr.device_args(*[ok] * 9)
    with pytest.raises(RuntimeError, match="argument 2 is not contiguous"):
        mr.device_args(ok, ok, torch.zeros(4, 4).t())
    with pytest.raises(RuntimeError, match="argument 1 is not a defined tensor"):
        mr.device_args(ok, None)
    assert mr.bound_device_args == []  # a rejected binding binds nothing
    gpu = _mr("cuda:0")  # the object alone needs no GPU
    with pytest.raises(RuntimeError, match="argument 0 is on cpu, this MapReduce's device is cuda:0"):
        gpu.device_args(ok)
    mr.device_args(*[ok] * 8)
    assert len(mr.bound_device_args) == 8
    mr.device_args()
    assert mr.bound_device_args == []


def test_scan_device_needs_a_gpu_mapreduce():
    mr = _mr("cpu")
    mr.map(1, lambda itask, kv: kv.add(b"k", b"v"))
    with pytest.raises(RuntimeError, match="GPU MapReduce"):
        mr.scan_device(SCAN_KV)


def test_args_keyword_restores_the_binding_after_an_exception():
    mr = _mr("cpu")
    a, b = torch.arange(3), torch.arange(5)
    mr.device_args(a)
    for call in (lambda: mr.map_device(10, MAP_TABLE, args=[b, a]),
                 lambda: mr.scan_device(SCAN_KV, args=[b]),
                 lambda: mr.sort_keys_device(SORTKEY_RANK, args=[b])):
        with pytest.raises(RuntimeError):  # a CPU MapReduce: every device call raises
            call()
        bound = mr.bound_device_args
        assert len(bound) == 1 and bound[0].data_ptr() == a.data_ptr()
    with pytest.raises(RuntimeError, match="argument 0 is not contiguous"):  # the keyword's own binding fails
        mr.map_device(10, MAP_TABLE, args=[torch.zeros(4, 4).t()])
    assert mr.bound_device_args[0].data_ptr() == a.data_ptr()
    assert mr.copy().bound_device_args == []  # copy() does not carry the binding


# ---------------------------------------------------------------------- GPU

def dev_i64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.int64)).cuda()


def kv_i64(mr):
    """the (int64 key, int64 value) pairs of a fixed-width KV, as two arrays"""
    kv = mr.kv
    assert kv.kw == 8 and kv.vw == 8
    return kv.kdata.view(torch.int64).cpu().numpy(), kv.vdata.view(torch.int64).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_map_tasks_reads_the_bound_table(n):
    mr = _mr("cuda")
    t = np.arange(n)
    tab = (np.arange(97) * 31 + 7) % 1009
    table, mod = dev_i64(tab), dev_i64([13])
    mr.device_args(table, mod)
    assert mr.map_device(n, MAP_TABLE) == n
    k, v = kv_i64(mr)
    assert (k == tab[t % 97] % 13).all() and (v == t).all()
    compiles = C.device_functor_compiles()
    tab2 = (np.arange(97) * 17 + 3) % 997
    table.copy_(dev_i64(tab2))  # new contents, the same tensor
    mod.fill_(11)
    assert mr.map_device(n, MAP_TABLE) == n
    k, v = kv_i64(mr)
    assert (k == tab2[t % 97] % 11).all() and (v == t).all()
    tab3 = np.arange(50) * 5 + 1  # a new tensor of another length, bound by keyword for this call
    assert mr.map_device(n, MAP_TABLE, args=[dev_i64(tab3), dev_i64([7])]) == n
    k, v = kv_i64(mr)
    assert (k == tab3[t % 50] % 7).all() and (v == t).all()
    assert C.device_functor_compiles() == compiles  # neither contents nor identity recompile
    assert mr.bound_device_args[0].data_ptr() == table.data_ptr()


@pytest.mark.gpu
def test_old_style_functor_under_a_binding():
    n = 3000
    mr = _mr("cuda")
    mr.device_args(dev_i64(range(10)))
    assert mr.map_device(n, old.GEN) == n + (n + 4) // 5
    mr.collate()
    assert mr.reduce_device(old.SUM_I32) == 97 + 89
    k, v = kv_i64(mr)
    t = np.arange(n)
    want = collections.Counter((t % 97).tolist())
    for x in t[t % 5 == 0]:
        want[int(x % 89 + 1000)] += 2
    assert dict(zip(k.tolist(), v.tolist())) == dict(want)


@pytest.mark.gpu
def test_args_past_the_bound_count_are_empty():
    mr = _mr("cuda")
    mr.device_args(dev_i64([1, 2, 3]), dev_i64([4]))
    assert mr.map_device(300, PAST) == 300
    k, v = kv_i64(mr)
    assert (k == np.arange(300)).all() and (v == 0).all()


@pytest.fixture(scope="module")
def keyed():
    """the oracle of the weighted reduces: key -> (sum + 1000) * w + w"""
    t = np.arange(N_KEYS_TASKS)
    key = np.where(t < 1000, t, np.where(t < 1256, 5, 6 + t % 900))
    val = t % 13 + 1
    w = np.arange(1000) % 5 + 1
    counts = np.bincount(key, minlength=1000)
    assert counts[0] == 1 and counts[1] == 1 and counts[5] == 257 and (counts > 0).all()
    sums = np.bincount(key, weights=val, minlength=1000).astype(np.int64)
    return w, {int(k): int((sums[k] + 1000) * w[k] + w[k]) for k in range(1000)}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["per-key", "fold"])
def test_reduce_reads_per_key_weights(keyed, form):
    w, want = keyed
    mr = _mr("cuda")
    mr.map_device(N_KEYS_TASKS, GEN_KEYS)
    assert mr.collate() == 1000
    assert mr.reduce_device(REDUCE_W if form == "per-key" else FOLD_W, args=[dev_i64(w)]) == 1000
    k, v = kv_i64(mr)
    assert dict(zip(k.tolist(), v.tolist())) == want


@pytest.mark.gpu
def test_compress_device_with_an_argument_on_variable_keys():
    rng = np.random.default_rng(1)
    vocab = ["a", "bb", "ccc", "dddd", "eeeee", "ff", "g" * 17]
    lines = [" ".join(rng.choice(vocab, size=rng.integers(0, 12))) for _ in range(500)]
    src = _mr("cuda")
    src.map(1, lambda itask, kv: [kv.add(struct.pack("<q", i), ln.encode()) for i, ln in enumerate(lines)])
    mr = _mr("cuda")
    mr.map_device(src, old.WORDS)
    mr.compress_device(COMPRESS_SCALE, args=[dev_i64([3])])
    want = collections.Counter(w for ln in lines for w in ln.split())
    got = {k.decode(): struct.unpack("<q", v)[0] for k, v in old.pairs(mr)}
    assert got == {w: 3 * c * len(w) for w, c in want.items()}


RANK = (np.arange(64) * 29 + 5) % 64  # a permutation of 0 .. 63 (29 is odd)


@pytest.mark.gpu
@pytest.mark.parametrize("code", [SORTKEY_RANK, COMPARE_RANK], ids=["sortkey", "compare"])
@pytest.mark.parametrize("n", [2, 2048, 2049])
def test_sort_keys_device_ranks_through_a_table(code, n):
    assert C.device_compare_tile() == 2048 and sorted(RANK.tolist()) == list(range(64))
    mr = _mr("cuda")
    mr.map_device(n, GEN_ROWS)
    assert mr.sort_keys_device(code, args=[dev_i64(RANK)]) == n
    k, v = kv_i64(mr)
    keys = (np.arange(n) * 37 + 11) % 64
    order = sorted(range(n), key=lambda i: RANK[keys[i]])  # Python's sort is stable
    assert v.tolist() == order and k.tolist() == keys[order].tolist()
    # the same rows with key and value swapped, sorted by value
    mr.map_device(n, GEN_ROWS_BY_VALUE)
    assert mr.sort_values_device(code, args=[dev_i64(RANK)]) == n
    k, v = kv_i64(mr)
    assert k.tolist() == order and v.tolist() == keys[order].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("code", [SORTKEY_RANK, COMPARE_RANK], ids=["sortkey", "compare"])
def test_sort_multivalues_device_ranks_through_a_table(code):
    n = 3 * 2049  # 2049 values a key, 6147 rows: tile sorts and merge passes
    mr = _mr("cuda")
    mr.map_device(n, GEN_MULTI)
    assert mr.collate() == 3
    assert mr.sort_multivalues_device(code, args=[dev_i64(RANK)]) == 3
    m = mr.kmv
    keys = m.keys.kdata.view(torch.int64).cpu().tolist()
    seg = m.seg.cpu().tolist()
    vals = m.vdata.view(torch.int64).view(-1, 2).cpu().numpy()
    assert sorted(keys) == [0, 1, 2]
    for j, key in enumerate(keys):
        rows = [t for t in range(n) if t % 3 == key]
        want = sorted(rows, key=lambda t: RANK[(t * 37 + 11) % 64])
        got = vals[seg[j]:seg[j + 1]]
        assert got[:, 1].tolist() == want and got[:, 0].tolist() == [(t * 37 + 11) % 64 for t in want]


def scan_oracle(n):
    t = np.arange(n)
    key = (t * 2654435761 >> 5) & 0xffff
    return np.bincount(key % 16, minlength=16)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 256, 70_000])
def test_scan_device_kv_visits_every_pair_once(n):
    mr = _mr("cuda")
    assert mr.map_device(n, GEN_SCAN) == n
    kd, vd = (mr.kv.kdata.clone(), mr.kv.vdata.clone()) if n else (None, None)
    acc, hist = dev_i64([0, 0, 0]), dev_i64([0] * 16)
    mr.device_args(acc, hist)
    assert mr.scan_device(SCAN_KV) == n
    assert acc.cpu().tolist() == [n, n * (n - 1) // 2, n]
    assert hist.cpu().tolist() == scan_oracle(n).tolist()
    if n:  # the data is bit-identical, in the same tensors
        assert mr.kv.n == n and torch.equal(mr.kv.kdata, kd) and torch.equal(mr.kv.vdata, vd)
    assert mr.scan_device(SCAN_KV) == n  # and again: the buffers accumulate
    assert acc.cpu().tolist() == [2 * n, n * (n - 1), 2 * n]


@pytest.mark.gpu
def test_scan_device_kmv():
    n = 5000
    mr = _mr("cuda")
    mr.map_device(n, GEN_GROUPS)
    assert mr.collate() == 10
    total, best = dev_i64([0]), dev_i64([-1] * 10)
    assert mr.scan_device(SCAN_KMV, args=[total, best]) == 10
    t = np.arange(n)
    key = np.where(t == 0, 0, np.where(t <= 1000, 1, 2 + t % 8))
    val = (t * 7919) % 100003
    assert (key == 0).sum() == 1 and (key == 1).sum() == 1000
    assert total.item() == n
    assert best.cpu().tolist() == [int(val[key == k].max()) for k in range(10)]
    assert mr.kmv is not None and mr.kmv.nkey == 10  # still a KMV
    with pytest.raises(RuntimeError, match="mr_scan"):  # the KV shape on a KMV
        mr.scan_device(SCAN_KV, args=[total, best])


def _budget(mr, data, tmp_path):
    mr.hbm_budget = data // 20
    mr.host_budget = data // 4
    mr.memsize = -65536
    mr.fpath = str(tmp_path)


@pytest.mark.gpu
def test_map_device_pieces_see_the_same_arguments(tmp_path):
    n = 50_000
    src = _mr("cuda")
    src.map_device(n, GEN_SCAN)
    tab = (np.arange(97) * 31 + 7) % 1009
    mr = _mr("cuda")
    _budget(mr, n * 16, tmp_path)  # pieces of 4096 pairs: 13 launches
    assert mr.map_device(src, MAP_PAIRS_TABLE, args=[dev_i64(tab)]) == n
    got = np.array([struct.unpack("<qq", k + v) for k, v in old.pairs(mr)])
    t = np.arange(n)
    assert (got[:, 0] == ((t * 2654435761 >> 5) & 0xffff)).all()
    assert (got[:, 1] == t + tab[t % 97]).all()


@pytest.mark.gpu
def test_scan_device_under_an_hbm_budget(tmp_path):
    n = 200_000
    mr = _mr("cuda")
    _budget(mr, n * 16, tmp_path)
    assert mr.map_device(n, GEN_SCAN) == n
    acc, hist = dev_i64([0, 0, 0]), dev_i64([0] * 16)
    assert mr.scan_device(SCAN_KV, args=[acc, hist]) == n
    assert acc.cpu().tolist() == [n, n * (n - 1) // 2, n]  # index = the pair's index on this rank, in every piece
    assert hist.cpu().tolist() == scan_oracle(n).tolist()
    assert mr.scan_device(SCAN_KV, args=[acc, hist]) == n  # the data is still there
    assert acc.cpu().tolist()[0] == 2 * n
