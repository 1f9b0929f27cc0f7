"""Device partitioner functor (csrc/engine/devfn.h, Kind::Hash): `mr_hash`,
MR-MPI's hash callback as device code, and its owner pass devfn::hash_dest.

Without a GPU: both signatures compile, a source without mr_hash is an error
that names it, a type error returns the compiler log. On the GPU, one process:
the owners C.device_hash_dest returns equal a NumPy evaluation of the same
function (fixed- and variable-width keys, zero-length keys, negative returns
and INT_MIN reduced as the host route of aggregate(hash) reduces them, a range
partitioner over bound splitters that never recompiles). Equality is exact."""
import struct

import numpy as np
import pytest
import torch

from gpu_mapreduce_amd import C

DEV = "cuda:0"
INT_MIN = -(1 << 31)

# ---------------------------------------------------------------------- sources

# 8-byte keys: k % 1000003
MOD = r"""
__device__ int mr_hash(mrd::Bytes key) { return (int)(key.as<unsigned long long>() % 1000003ull); }
"""
# negative returns: -(k % 5) - 1, and INT_MIN for every k that 11 divides
NEG = r"""
__device__ int mr_hash(mrd::Bytes key) {
  const unsigned long long k = key.as<unsigned long long>();
  return k % 11 == 0 ? -2147483647 - 1 : -(int)(k % 5) - 1;
}
"""
# any width, zero included: length and first byte
LEN_FIRST = r"""
__device__ int mr_hash(mrd::Bytes key) { return (int)(key.n * 31 + (key.n ? key.p[0] : 7)); }
"""
# the bound-buffer form that reads nothing: the number of bound buffers
NARGS = r"""
__device__ int mr_hash(mrd::Bytes key, const mrd::Args& args) { return args.n; }
"""
# a range partitioner: owner = the number of splitters <= key (args[0]: ascending uint64)
RANGE = r"""
__device__ int mr_hash(mrd::Bytes key, const mrd::Args& args) {
  const unsigned long long* s = args[0].as<unsigned long long>();
  const unsigned long long k = key.as<unsigned long long>();
  long long lo = 0, hi = args[0].count<unsigned long long>();
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (s[mid] <= k) lo = mid + 1;
    else hi = mid;
  }
  return (int)lo;
}
"""
NO_HASH = "__device__ int other(mrd::Bytes key) { return 0; }\n"
TYPE_ERROR = "__device__ int mr_hash(mrd::Bytes key) { return key.no_such_member; }\n"


def mod_np(k):
    return (k.astype(np.uint64) % np.uint64(1000003)).astype(np.int64)


def neg_np(k):
    k = k.astype(np.uint64)
    return np.where(k % np.uint64(11) == 0, INT_MIN, -(k % np.uint64(5)).astype(np.int64) - 1)


def owner_np(h, P):
    """((long long)h % P + P) % P, in int64 (NumPy's % is already the floored one)"""
    return (np.asarray(h, dtype=np.int64) % P + P) % P


def neg_py(key):
    k = struct.unpack("<Q", key)[0]
    return INT_MIN if k % 11 == 0 else -(k % 5) - 1


def len_first_py(key):
    return len(key) * 31 + (key[0] if key else 7)


# ---------------------------------------------------------------------- no GPU

def test_both_signatures_compile_and_every_check_counts():
    before = C.device_functor_compiles()
    assert C.device_hash_check(MOD) > 0
    assert C.device_hash_check(NARGS) > 0
    assert C.device_hash_check(NEG) > 0
    assert C.device_hash_check(LEN_FIRST) > 0
    assert C.device_hash_check(RANGE) > 0
    assert C.device_functor_compiles() == before + 5


def test_source_without_mr_hash_names_it():
    with pytest.raises(RuntimeError, match="mr_hash"):
        C.device_hash_check(NO_HASH)
    with pytest.raises(RuntimeError, match="mr_hash"):  # another kind's functor is not a partitioner
        C.device_hash_check("__device__ unsigned long long mr_sortkey(mrd::Bytes b) { return 0; }")


def test_type_error_returns_the_compiler_log():
    with pytest.raises(RuntimeError, match=r"does not compile:(.|\n)*mrd_hash\.hip(.|\n)*no_such_member"):
        C.device_hash_check(TYPE_ERROR)
    with pytest.raises(RuntimeError, match="does not compile"):  # a key that is not mrd::Bytes
        C.device_hash_check("__device__ int mr_hash(int key) { return key; }")


# ---------------------------------------------------------------------- GPU, one process

def fixed_kv(k):
    k = np.ascontiguousarray(k)
    return C.make_kv(torch.from_numpy(k.view(np.uint8)), None, torch.empty(0, dtype=torch.uint8), None, len(k), DEV)


def var_kv(keys):
    off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    data = torch.frombuffer(bytearray(b"".join(keys)), dtype=torch.uint8) if off[-1] else torch.empty(0, dtype=torch.uint8)
    return C.make_kv(data, torch.from_numpy(off), torch.empty(0, dtype=torch.uint8), None, len(keys), DEV)


def owners(kv, P, code, args=()):
    d = C.device_hash_dest(kv, P, code, list(args))
    assert d.dtype == torch.int32 and d.is_cuda and d.shape == (kv.n,)
    return d.cpu().numpy().astype(np.int64)


WORLDS = [1, 2, 3, 7, 1024]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 257, 70_001])
def test_fixed_width_owners_match_numpy(n):
    k = np.random.default_rng(n).integers(0, 1 << 63, n, dtype=np.int64).view(np.uint64)
    kv = fixed_kv(k)
    for P in WORLDS:
        assert (owners(kv, P, MOD) == mod_np(k) % P).all(), P


@pytest.mark.gpu
def test_negative_returns_and_int_min_land_where_the_host_route_puts_them():
    k = np.arange(70_001, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(7)
    h = neg_np(k)
    assert (h == INT_MIN).sum() > 1000 and sorted(set(h.tolist()) - {INT_MIN}) == [-5, -4, -3, -2, -1]
    kv = fixed_kv(k)
    for P in WORLDS:
        got = owners(kv, P, NEG)
        assert (got == owner_np(h, P)).all() and got.min() >= 0 and got.max() < P, P
        # the arithmetic host_dest does, pair by pair, on a sample
        assert got[:500].tolist() == [((neg_py(struct.pack("<Q", int(x))) % P) + P) % P for x in k[:500]]


@pytest.mark.gpu
def test_variable_width_and_zero_length_keys():
    rng = np.random.default_rng(5)
    keys = [bytes(rng.integers(0, 256, rng.integers(0, 40), dtype=np.uint8)) for _ in range(3000)]
    for i in (0, 1, 77, 78, 1500, len(keys) - 1):  # zero-length keys, first and last row among them, two adjacent
        keys[i] = b""
    h = np.array([len_first_py(k) for k in keys])
    assert (h == 7).sum() >= 6 and len(set(h.tolist())) > 500
    kv = var_kv(keys)
    assert kv.kw == -1
    for P in WORLDS:
        assert (owners(kv, P, LEN_FIRST) == h % P).all(), P
    # every key empty: no key byte at all behind the offsets; and the fixed width 0
    assert (owners(var_kv([b""] * 300), 5, LEN_FIRST) == 7 % 5).all()
    zero = C.make_kv(torch.empty(0, dtype=torch.uint8), None, torch.arange(300).view(torch.uint8), None, 300, DEV)
    assert zero.kw == 0 and (owners(zero, 5, LEN_FIRST) == 7 % 5).all()


@pytest.mark.gpu
def test_range_partitioner_reads_bound_splitters_without_recompiling():
    code = RANGE + "// test_range_partitioner\n"  # a source no other test has loaded
    rng = np.random.default_rng(9)
    k = rng.integers(0, 1 << 63, 70_001, dtype=np.int64).view(np.uint64) * np.uint64(2)  # up to 2^64
    k[0], k[1], k[2] = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1 << 63)
    kv = fixed_kv(k)

    def dev_u64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)

    s1 = np.sort(rng.integers(0, 1 << 63, 6, dtype=np.int64).view(np.uint64) * np.uint64(2))
    s1[2] = k[100]  # a key equal to a splitter belongs to the range above it
    s1.sort()
    s2 = np.quantile(k.astype(np.float64), np.arange(1, 7) / 7).astype(np.uint64)
    before = C.device_functor_compiles()
    split = dev_u64(s1)
    got1 = owners(kv, 7, code, [split])
    split.copy_(dev_u64(s2))  # new contents, the same tensor
    got2 = owners(kv, 7, code, [split])
    s3 = np.sort(k[::70])[::100][1:]  # another tensor of another length: 10 splitters, 11 ranks
    got3 = owners(kv, len(s3) + 1, code, [dev_u64(s3)])
    assert C.device_functor_compiles() == before + 1
    for got, s in ((got1, s1), (got2, s2), (got3, s3)):
        assert (got == np.searchsorted(s, k, side="right")).all()
    assert got1[100] == np.searchsorted(s1, k[100], side="right") and not (got1 == got2).all()
    assert np.bincount(got2, minlength=7).min() > 70_001 // 7 * 0.9  # quantiles: no rank short of pairs
    # no buffer bound: count() is 0, every key belongs to rank 0
    assert (owners(kv, 7, code) == 0).all()
    assert C.device_functor_compiles() == before + 1

