"""Device comparator functors (csrc/engine/devfn.cpp, kind mrd_compare.hip):
`__device__ int mr_compare(mrd::Bytes a, mrd::Bytes b)` drives a stable merge
sort on the GPU for sort_keys_device / sort_values_device /
sort_multivalues_device. Compilation, the tile constant and the CPU-engine
error are checked without a GPU; the sorts are checked on the GPU against
Python's stable `sorted(..., key=cmp_to_key(...))`, the whole (key, value)
list compared exactly with value = input row number, so tie order counts.

The GPU tests share four functor sources (tests/functors/*.hip): each costs
one run-time compile."""
import functools
import os
import struct

import numpy as np
import pytest

from gpu_mapreduce_amd import C

FUNCTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "functors")


def functor(name):
    with open(os.path.join(FUNCTORS, name)) as f:
        return f.read()


CMP16 = functor("cmp16.hip")          # (int64 a, int64 b): b descending, a ascending
CMPSTR = functor("cmpstr.hip")        # byte strings: longer first, then bytes ascending
CMP12 = functor("cmp12.hip")          # {int a, int b, uint tag}: a descending, b ascending
SORTKEY12 = functor("sortkey12.hip")  # the same order as a 64-bit key (+ a helper named mr_compare)


def sign(x):
    return -1 if x < 0 else 1 if x > 0 else 0


def pycmp16(x, y):  # on the unpacked (a, b)
    return sign(y[1] - x[1]) or sign(x[0] - y[0])


def pycmpstr(x, y):
    x, y = bytes(x), bytes(y)
    return sign(len(y) - len(x)) or (-1 if x < y else 1 if x > y else 0)


def pycmp12(x, y):
    xa, xb, _ = struct.unpack("<iiI", x)
    ya, yb, _ = struct.unpack("<iiI", y)
    return sign(ya - xa) or sign(xb - yb)


# ---------------------------------------------------------------------- no GPU

def test_compare_functor_compiles_and_reports_errors():
    assert C.device_compare_check(CMP16) > 0
    assert C.device_compare_check(CMPSTR) > 0
    with pytest.raises(RuntimeError, match="does not compile") as e:
        C.device_compare_check("__device__ int mr_compare(mrd::Bytes a, mrd::Bytes b) { return undeclared_name; }")
    assert "undeclared_name" in str(e.value)  # the compiler log comes with it


def test_compare_tile_is_a_power_of_two():
    t = C.device_compare_tile()
    assert t >= 256 and t & (t - 1) == 0


def _cpu_mr(npairs):
    from gpu_mapreduce_amd.parallel.comm import Comm
    from gpu_mapreduce_amd.runtime.mapreduce import MapReduce
    mr = MapReduce(Comm(device="cpu"))
    mr.map(1, lambda itask, kv: kv.add_multi_static([struct.pack("<qq", i % 3, i % 5) for i in range(npairs)],
                                                    [struct.pack("<q", i) for i in range(npairs)]))
    return mr


def test_compare_functor_needs_a_gpu_mapreduce():
    mr = _cpu_mr(10)
    with pytest.raises(RuntimeError, match="GPU MapReduce"):
        mr.sort_keys_device(CMP16)
    mr.collate()
    with pytest.raises(RuntimeError, match="GPU MapReduce"):
        mr.sort_multivalues_device(CMP16)


def test_sort_functor_with_neither_name_is_an_error():
    mr = _cpu_mr(10)
    with pytest.raises(RuntimeError, match="mr_sortkey.*mr_compare"):
        mr.sort_keys_device("__device__ int my_order(mrd::Bytes a, mrd::Bytes b) { return 0; }")


# ------------------------------------------------------------------------- GPU

def gpu_mr():
    from gpu_mapreduce_amd.parallel.comm import Comm
    from gpu_mapreduce_amd.runtime.mapreduce import MapReduce
    return MapReduce(Comm(device="cuda"))


def fill(mr, keys, values, fixed=True):
    def m(itask, kv):
        if not keys:
            return
        (kv.add_multi_static if fixed else kv.add_multi_dynamic)(keys, values)
    mr.map(1, m)


def pairs(mr):
    out = []
    mr.scan_kv(lambda k, v: out.append((bytes(k), bytes(v))))
    return out


def rows16(n, seed, kind="random"):
    rng = np.random.default_rng(seed)
    a = rng.integers(-6, 6, n)
    b = rng.integers(-4, 4, n)  # small ranges: ties are common
    rows = [(int(x), int(y)) for x, y in zip(a, b)]
    if kind == "equal":
        rows = [(3, -2)] * n
    elif kind == "sorted":
        rows.sort(key=functools.cmp_to_key(pycmp16))
    elif kind == "reverse":
        rows.sort(key=functools.cmp_to_key(pycmp16), reverse=True)
    return rows


def pack16(rows):
    return [struct.pack("<qq", a, b) for a, b in rows]


def tags(n):
    return [struct.pack("<q", i) for i in range(n)]


def check_sort_keys16(n, seed, kind="random"):
    rows, vals = rows16(n, seed, kind), tags(n)
    mr = gpu_mr()
    fill(mr, pack16(rows), vals)
    assert mr.sort_keys_device(CMP16) == n
    want = sorted(zip(rows, vals), key=functools.cmp_to_key(lambda p, q: pycmp16(p[0], q[0])))
    want = list(zip(pack16(r for r, _ in want), (v for _, v in want)))
    assert pairs(mr) == want
    return want


T = C.device_compare_tile()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5, 5 * T + 3],
                         ids=["0", "1", "2", "T-1", "T", "T+1", "2T+1", "3T+5", "5T+3"])
def test_sort_keys_fixed16(n):
    """the trivial sizes, the tile edge, and a run without a partner at the
    first (2T+1), second (3T+5) and third (5T+3) merge level"""
    check_sort_keys16(n, seed=n + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["equal", "sorted", "reverse"])
def test_sort_keys_fixed16_orders(kind):
    n = 3 * T + 5
    want = check_sort_keys16(n, seed=11, kind=kind)
    if kind == "equal":  # all ties: the identity
        assert [v for _, v in want] == tags(n)


@pytest.mark.gpu
def test_sort_keys_variable_width_and_host_path_agree():
    n = 2 * T + 1
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 25, n)
    lens[[0, 7, n // 2, n - 1]] = 0  # several empty keys, first and last row among them
    keys = [bytes(rng.integers(97, 100, int(ln), dtype=np.uint8)) for ln in lens]
    vals = tags(n)
    want = sorted(zip(keys, vals), key=functools.cmp_to_key(lambda p, q: pycmpstr(p[0], q[0])))
    mr = gpu_mr()
    fill(mr, keys, vals, fixed=False)
    assert mr.sort_keys_device(CMPSTR) == n
    got = pairs(mr)
    assert got == want
    host = gpu_mr()  # the same data through the host comparator path
    m = min(n, 4096)
    fill(host, keys[:m], vals[:m], fixed=False)
    host.sort_keys(pycmpstr)
    dev = gpu_mr()
    fill(dev, keys[:m], vals[:m], fixed=False)
    dev.sort_keys_device(CMPSTR)
    assert pairs(host) == pairs(dev)


@pytest.mark.gpu
def test_sort_values_fixed16():
    n = 2 * T + 1
    rows, ks = rows16(n, seed=21), tags(n)
    mr = gpu_mr()
    fill(mr, ks, pack16(rows))
    assert mr.sort_values_device(CMP16) == n
    want = sorted(zip(ks, rows), key=functools.cmp_to_key(lambda p, q: pycmp16(p[1], q[1])))
    assert pairs(mr) == list(zip((k for k, _ in want), pack16(r for _, r in want)))


def kmv_lists(mr):
    out = []
    mr.scan_kmv(lambda k, vals: out.append((bytes(k), [bytes(v) for v in vals])))
    return out


@pytest.fixture(scope="module")
def multivalue_case():
    """(keys, values) of a KV whose collate gives segments of 1, 2, T, T + 1,
    2T + 3 and a few mid-sized value counts, the first segment exactly one
    tile (an edge on a tile edge) and the others ending inside tiles. The key
    order of a KMV is the engine's (hash order), so a pilot collate learns it."""
    counts = [T, 37, 1, 2, T + 1, 700, 2 * T + 3, 45, 300]
    ids = list(range(100, 100 + len(counts)))
    pilot = gpu_mr()
    fill(pilot, [struct.pack("<q", i) for i in ids], [b"\0" * 12] * len(ids))
    pilot.collate()
    order = [struct.unpack("<q", k)[0] for k, _ in kmv_lists(pilot)]
    assert sorted(order) == ids
    count_of = dict(zip(order, counts))
    rng = np.random.default_rng(9)
    keys, vals = [], []
    owner = rng.permutation(np.repeat(ids, [count_of[i] for i in ids]))  # the keys' pairs interleaved
    a = rng.integers(-3, 3, len(owner))
    b = rng.integers(-5, 5, len(owner))
    for r, (o, x, y) in enumerate(zip(owner, a, b)):
        keys.append(struct.pack("<q", int(o)))
        vals.append(struct.pack("<iiI", int(x), int(y), r))
    return keys, vals, [count_of[i] for i in order]


@pytest.mark.gpu
@pytest.mark.parametrize("code", ["mr_compare", "mr_sortkey"])
def test_sort_multivalues_device(multivalue_case, code):
    keys, vals, counts = multivalue_case
    mr = gpu_mr()
    fill(mr, keys, vals)
    nkey = mr.collate()
    before = kmv_lists(mr)
    assert [len(v) for _, v in before] == counts
    edges = np.cumsum(counts)[:-1]
    assert (edges % T == 0).any() and (edges % T != 0).any()
    assert mr.sort_multivalues_device(CMP12 if code == "mr_compare" else SORTKEY12) == nkey == len(counts)
    after = kmv_lists(mr)
    assert [k for k, _ in after] == [k for k, _ in before]  # the key order is unchanged
    for (k, got), (_, had) in zip(after, before):
        assert got == sorted(had, key=functools.cmp_to_key(pycmp12)), k


@pytest.mark.gpu
def test_sortkey_code_keeps_the_radix_route():
    """code that defines mr_sortkey takes the radix sort even when a helper of
    it is named mr_compare (here one that orders the other way round)"""
    n = 3000
    rng = np.random.default_rng(3)
    rows = [struct.pack("<iiI", int(x), int(y), i)
            for i, (x, y) in enumerate(zip(rng.integers(-9, 9, n), rng.integers(-9, 9, n)))]
    vals = tags(n)
    mr = gpu_mr()
    fill(mr, rows, vals)
    assert mr.sort_keys_device(SORTKEY12) == n
    want = sorted(zip(rows, vals), key=functools.cmp_to_key(lambda p, q: pycmp12(p[0], q[0])))
    assert pairs(mr) == want


@pytest.mark.gpu
def test_sort_keys_fixed16_several_merge_levels():
    check_sort_keys16(100_000, seed=77)
