"""print_device / text_device (csrc/engine/devfn.h, Kind::Print): the pairs of a
KV or the keys of a KMV formatted to text on the GPU by `mr_print`, through
`mrd::Text`.

Without a GPU: both shapes compile with and without the bound buffers, a
source without mr_print and a type error are reported, a CPU MapReduce refuses
the ops, and `print` (whose file and rank tail the new op shares) still writes
the bytes it wrote before that tail became a helper. On the GPU every oracle
is Python `bytes` built on the host from what the KV / KMV holds, and equality
is exact. The routes of the write kernel (a tile's text staged in LDS, or
written straight to HBM) are asserted through C.device_text_tiles()."""
import importlib.util
import io
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_mapreduce_amd import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu_mapreduce_amd")
EXAMPLE = os.path.join(ROOT, "examples", "python", "inverted_index_print_device.py")
STAGE = 32768
TILE = 256

# ---------------------------------------------------------------------- sources

# task t -> (int64 t * 7 + 1, int64 t * t)
GEN = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  out.emit((long long)(t * 7 + 1), (long long)(t * t));
}
"""
# "<index> <key hex> <value>\n" of two int64
KV_LINE = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out) {
  out.dec(index);
  out.chr(' ');
  out.hex(key.as<unsigned long long>());
  out.chr(' ');
  out.dec(value.as<long long>());
  out.chr('\n');
}
"""
# any widths: "<index>:<key bytes>=<value bytes>;"
KV_RAW = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out) {
  out.dec(index);
  out.chr(':');
  out.put(key);
  out.chr('=');
  out.put(value.p, value.n);
  out.chr(';');
}
"""
KV_ARGS = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out, const mrd::Args& args) {
  out.dec(args[0].as<long long>()[index % args[0].count<long long>()]);
  out.chr('\n');
}
"""
# "<key bytes>[<n>]: v v v\n", the values as raw bytes
KMV_RAW = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Values vals, mrd::Text& out) {
  out.put(key);
  out.chr('[');
  out.dec(vals.n);
  out.str("]:");
  for (long long i = 0; i < vals.n; ++i) {
    out.chr(' ');
    out.put(vals[i]);
  }
  out.chr('\n');
}
"""
# int64 keys, int32 values: "<key>\t<v> <v> ...\n"
KMV_INTS = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Values vals, mrd::Text& out) {
  out.dec(key.as<long long>());
  out.chr('\t');
  for (long long i = 0; i < vals.n; ++i) {
    if (i) out.chr(' ');
    out.dec(vals.get<int>(i));
  }
  out.chr('\n');
}
"""
KMV_ARGS = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Values vals, mrd::Text& out, const mrd::Args& args) {
  out.udec(args[0].n + vals.n);
}
"""
NO_PRINT = GEN
TYPE_ERROR = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out) {
  out.no_such_member(1);
}
"""
# every member of mrd::Text once, the cases in the bound buffers:
# args[0] int64 for dec, args[1] uint64 for udec and hex, args[2] float64 x and args[3] int32 d for fixed
MEMBERS = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out, const mrd::Args& args) {
  for (long long i = 0; i < args[0].count<long long>(); ++i) {
    out.dec(args[0].as<long long>()[i]);
    out.chr('\n');
  }
  for (long long i = 0; i < args[1].count<unsigned long long>(); ++i) {
    out.udec(args[1].as<unsigned long long>()[i]);
    out.chr(' ');
    out.hex(args[1].as<unsigned long long>()[i]);
    out.chr('\n');
  }
  for (long long i = 0; i < args[2].count<double>(); ++i) {
    out.fixed(args[2].as<double>()[i], args[3].as<int>()[i]);
    out.chr('\n');
  }
  out.put(key.p, 0);
  out.put(mrd::Bytes{nullptr, 0});
  out.str("");
  out.str("end");
}
"""
# pair t writes nothing when t % 3 == 0
SOME = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out) {
  if (index % 3 == 0) return;
  out.dec(index);
  out.chr(',');
}
"""
# the whole second tile writes nothing
NOT_TILE_1 = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out) {
  if (index / 256 == 1) return;
  out.dec(index);
  out.chr(',');
}
"""
# pair t writes args[0][t] bytes, the letter of t
LENGTHS = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out, const mrd::Args& args) {
  const long long n = args[0].as<long long>()[index];
  for (long long i = 0; i < n; ++i) out.chr((char)('a' + index % 26));
}
"""
# one byte a pair: a 1-byte key, no value
GEN_BYTE = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  out.emit_key((char)1);
}
"""
DIGIT = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out) {
  out.dec(index % 10);
  out.chr('\n');
}
"""
# 41 000 tasks: keys 1000 .. 1499 and 41 500 .. 41 999 hold one int32 value, key 7 holds 40 000
GEN_HOT = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  const long long k = t < 500 ? 1000 + t : t < 40500 ? 7 : 1000 + t;
  out.emit(k, (int)(t % 1000003));
}
"""
# groups for the out-of-core run: 3000 keys of 1 .. 6 int32 values
GEN_GROUPS = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  out.emit((long long)(t % 3000), (int)(t * 31 % 1009));
  if (t % 2 == 0) out.emit((long long)((t / 2) % 3000), (int)(t % 17));
}
"""


# ---------------------------------------------------------------------- helpers and oracles

def _mr(device):
    from gpu_mapreduce_amd.parallel.comm import Comm
    from gpu_mapreduce_amd.runtime.mapreduce import MapReduce
    return MapReduce(Comm(device=device))


def _rows(data, off, w, n):
    """the n rows of a column as bytes"""
    d = data.cpu().numpy().tobytes() if data is not None and data.numel() else b""
    if w >= 0:
        return [d[i * w:(i + 1) * w] for i in range(n)]
    o = off.cpu().tolist()
    return [d[o[i]:o[i + 1]] for i in range(n)]


def kv_items(mr):
    kv = mr.kv
    return list(zip(_rows(kv.kdata, kv.koff, kv.kw, kv.n), _rows(kv.vdata, kv.voff, kv.vw, kv.n)))


def kmv_items(mr):
    m = mr.kmv
    keys = _rows(m.keys.kdata, m.keys.koff, m.keys.kw, m.nkey)
    vals = _rows(m.vdata, m.voff, m.vw, m.nval)
    seg = m.seg.cpu().tolist()
    return [(keys[i], vals[seg[i]:seg[i + 1]]) for i in range(m.nkey)]


def text_of(mr, code, args=None):
    t = mr.text_device(code, args=args)
    assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1
    return t.cpu().numpy().tobytes()


def line_kv(i, k, v):
    return b"%d %x %d\n" % (i, struct.unpack("<Q", k)[0], struct.unpack("<q", v)[0])


def raw_kv(i, k, v):
    return b"%d:" % i + k + b"=" + v + b";"


def raw_kmv(k, vals):
    return k + b"[%d]:" % len(vals) + b"".join(b" " + v for v in vals) + b"\n"


def ints_kmv(k, vals):
    return b"%d\t" % struct.unpack("<q", k)[0] + b" ".join(b"%d" % struct.unpack("<i", v)[0] for v in vals) + b"\n"


def py_fixed(x, d):
    """mrd::Text::fixed, as devfn.h defines it"""
    d = min(max(d, 0), 9)
    if x != x:
        return "nan"
    neg = x < 0
    if math.isinf(x):
        return "-inf" if neg else "inf"
    m = abs(x) * 10.0 ** d  # one IEEE multiply by an exact power
    if m >= 2.0 ** 63:
        return "-ovf" if neg else "ovf"
    n = round(m)  # half-even, exact
    s = "-" if neg and n else ""
    s += str(n // 10 ** d)
    if d:
        s += "." + str(n % 10 ** d).zfill(d)
    return s


def tiles():
    return np.array(C.device_text_tiles(), dtype=np.int64)


def routes_of(lengths):
    """(staged, direct) tiles of a launch over items with these text lengths"""
    staged = direct = 0
    for t in range(0, len(lengths), TILE):
        if sum(lengths[t:t + TILE]) <= STAGE:
            staged += 1
        else:
            direct += 1
    return np.array([staged, direct])


def cuda_i64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.int64)).cuda()


# ---------------------------------------------------------------------- without a GPU

def test_print_functor_compiles_in_both_shapes_with_and_without_args():
    before = C.device_functor_compiles()
    assert C.device_print_check(KV_LINE, False) > 0
    assert C.device_print_check(KV_ARGS, False) > 0
    assert C.device_print_check(KMV_RAW, True) > 0
    assert C.device_print_check(KMV_ARGS, True) > 0
    assert C.device_print_check(MEMBERS, False) > 0
    assert C.device_functor_compiles() == before + 5
    assert C.device_text_stage_bytes() == STAGE


def test_print_functor_errors():
    with pytest.raises(RuntimeError, match="has no mr_print"):
        C.device_print_check(NO_PRINT, False)
    with pytest.raises(RuntimeError, match="does not compile(.|\n)*no_such_member"):
        C.device_print_check(TYPE_ERROR, False)
    with pytest.raises(RuntimeError, match="does not compile"):  # the KV shape where the KMV one is asked for
        C.device_print_check(KV_LINE, True)


def test_print_device_needs_a_gpu_mapreduce(tmp_path):
    mr = _mr("cpu")
    mr.map(1, lambda itask, kv: kv.add(b"k", b"v"))
    with pytest.raises(RuntimeError, match="device functors run on a GPU MapReduce"):
        mr.text_device(KV_LINE)
    with pytest.raises(RuntimeError, match="device functors run on a GPU MapReduce"):
        mr.print_device(str(tmp_path / "t"), 0, -1, KV_LINE)
    assert not (tmp_path / "t").exists()


# what `print` wrote for these pairs before its file / rank tail became the
# helper it now shares with print_device (recorded from the parent commit)
PRINT_KV = (b"KV pair: proc 0, sizes 4 8, key 1, value alpha  \n"
            b"KV pair: proc 0, sizes 4 8, key 2, value beta   \n"
            b"KV pair: proc 0, sizes 4 8, key 3, value gamma  \n")
PRINT_KV_STRIDE2 = b"KV pair: proc 0, sizes 4 8, key 2, value beta   \n"
PRINT_KMV = (b"KMV pair: proc 0, nvalues 2, sizes 4 16, key 1, values alpha    beta     \n"
             b"KMV pair: proc 0, nvalues 1, sizes 4 8, key 2, values gamma    \n")


def _print_mr(kmv=False):
    mr = _mr("cpu")
    pairs = [(1, b"alpha  \0"), (2, b"beta   \0"), (3, b"gamma  \0")]
    if kmv:
        pairs = [(1, b"alpha   "), (1, b"beta    "), (2, b"gamma   ")]
    mr.map(1, lambda itask, kv: [kv.add(struct.pack("<i", k), v) for k, v in pairs])
    if kmv:
        mr.convert()
    return mr


def test_print_on_the_cpu_engine_writes_what_it_wrote(tmp_path, capsys):
    mr = _print_mr()
    f = str(tmp_path / "kv.txt")
    mr.print(-1, 1, 1, 5, file=f, fflag=0)
    assert open(f, "rb").read() == PRINT_KV
    mr.print(0, 1, 1, 5, file=f, fflag=0)  # proc 0: this rank
    assert open(f, "rb").read() == PRINT_KV
    mr.print(-1, 2, 1, 5, file=f, fflag=1)  # fflag 1: file.<rank>
    assert open(f + ".0", "rb").read() == PRINT_KV_STRIDE2
    g = str(tmp_path / "none.txt")
    mr.print(1, 1, 1, 5, file=g, fflag=0)  # proc 1: another rank's turn
    assert not os.path.exists(g)
    capsys.readouterr()
    mr.print(-1, 1, 1, 5)
    assert capsys.readouterr().out.encode() == PRINT_KV
    mr.print(1, 1, 1, 5)
    assert capsys.readouterr().out == ""
    m = _print_mr(kmv=True)
    m.print(-1, 1, 1, 5, file=f, fflag=0)
    assert open(f, "rb").read() == PRINT_KMV
    with pytest.raises(RuntimeError, match="Could not open print file"):
        mr.print(-1, 1, 1, 5, file=str(tmp_path / "no" / "such" / "dir.txt"), fflag=0)


# ---------------------------------------------------------------------- GPU: mrd::Text

DEC = [0, 1, -1, 9, -9, 10, -10, -2 ** 63, 2 ** 63 - 1]
UNS = [0, 0xf, 0x10, 2 ** 64 - 1]
FIXED = [(0.5, 0), (1.5, 0), (2.5, 0), (0.125, 2), (0.375, 2), (-0.0, 0), (-0.004, 2), (1e-9, 9), (float("nan"), 3),
         (float("inf"), 1), (float("-inf"), 1), (1e19, 0), (-1e19, 0), (2.25, -1), (1.0000000004, 12), (-1234.5678, 3),
         (9.2e18, 0), (123456789.987654321, 9)]


@pytest.mark.gpu
def test_text_members_equal_the_python_definition():
    assert [py_fixed(x, d) for x, d in FIXED[:8]] == ["0", "2", "2", "0.12", "0.38", "0", "0.00", "0.000000001"]
    assert py_fixed(1e19, 0) == "ovf" and py_fixed(2.25, -1) == "2" and py_fixed(1.0000000004, 12) == "1.000000000"
    mr = _mr("cuda")
    assert mr.map_device(1, GEN) == 1
    args = [cuda_i64(DEC), torch.as_tensor(np.array(UNS, dtype=np.uint64).view(np.int64)).cuda(),
            torch.tensor([x for x, _ in FIXED], dtype=torch.float64).cuda(),
            torch.tensor([d for _, d in FIXED], dtype=torch.int32).cuda()]
    want = "".join("%d\n" % v for v in DEC) + "".join("%d %x\n" % (v, v) for v in UNS)
    want += "".join(py_fixed(x, d) + "\n" for x, d in FIXED) + "end"
    assert text_of(mr, MEMBERS, args=args) == want.encode()


# ---------------------------------------------------------------------- GPU: item counts, shapes

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_text_of_n_pairs(n, tmp_path):
    mr = _mr("cuda")
    assert mr.map_device(n, GEN) == n
    want = b"".join(line_kv(i, struct.pack("<q", i * 7 + 1), struct.pack("<q", i * i)) for i in range(n))
    assert text_of(mr, KV_LINE) == want
    f = str(tmp_path / "out.txt")
    assert mr.print_device(f, 0, -1, KV_LINE) == len(want)  # n == 0: an empty file, 0 bytes
    assert open(f, "rb").read() == want


@pytest.mark.gpu
def test_more_items_than_one_grid_sweep():
    n = 2 ** 24 + 257  # 65 538 tiles for the write kernel's 65 536 workgroups, and a count grid that strides
    mr = _mr("cuda")
    assert mr.map_device(n, GEN_BYTE) == n
    before = tiles()
    got = mr.text_device(DIGIT)
    want = np.empty(2 * n, dtype=np.uint8)
    want[0::2] = 48 + np.arange(n) % 10
    want[1::2] = 10
    assert got.numel() == 2 * n and torch.equal(got, torch.from_numpy(want).cuda())
    assert (tiles() - before).tolist() == [-(-n // TILE), 0] == [65538, 0]


def _host_mr(pairs):
    mr = _mr("cuda")
    mr.map(1, lambda itask, kv: [kv.add(k, v) for k, v in pairs])
    return mr


@pytest.mark.gpu
def test_variable_and_zero_length_keys_and_values():
    rng = np.random.default_rng(7)
    words = [b"", b"a", b"bb", b"hello world", b"x" * 37]
    pairs = [(words[int(rng.integers(0, 5))], words[int(rng.integers(0, 5))]) for _ in range(600)]
    mr = _host_mr(pairs)
    assert kv_items(mr) == pairs
    assert text_of(mr, KV_RAW) == b"".join(raw_kv(i, k, v) for i, (k, v) in enumerate(pairs))
    # every key empty / every value empty
    for pairs in ([(b"", b"v%d" % i) for i in range(300)], [(b"key%d" % i, b"") for i in range(300)]):
        mr = _host_mr(pairs)
        assert text_of(mr, KV_RAW) == b"".join(raw_kv(i, k, v) for i, (k, v) in enumerate(pairs))


@pytest.mark.gpu
def test_items_and_a_whole_tile_that_write_nothing():
    n = 700
    mr = _mr("cuda")
    mr.map_device(n, GEN)
    assert text_of(mr, SOME) == b"".join(b"%d," % i for i in range(n) if i % 3)
    before = tiles()
    assert text_of(mr, NOT_TILE_1) == b"".join(b"%d," % i for i in range(n) if i // 256 != 1)
    assert (tiles() - before).sum() == 3
    assert text_of(mr, NOT_TILE_1.replace("== 1", ">= 0")) == b""  # nothing at all


# ---------------------------------------------------------------------- GPU: routes

@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 5])
def test_tiles_at_the_stage_size_take_the_route_their_total_says(lead, monkeypatch):
    """tile totals of STAGE - 1, STAGE, STAGE + 1 and a short last tile; the
    second tile's text starts at byte STAGE - 1 of the output (not on a
    16-byte line), and with lead the whole text starts 5 bytes into its
    allocation, so every tile does"""
    assert C.device_text_stage_bytes() == STAGE
    lengths = []
    for total in (STAGE - 1, STAGE, STAGE + 1):
        lengths += [total - 3 * (TILE - 1)] + [3] * (TILE - 1)
    lengths += [1, 0, 40, 7] * 10
    n = len(lengths)
    monkeypatch.setenv("MRH_TEXT_LEAD", str(lead))
    mr = _mr("cuda")
    mr.map_device(n, GEN)
    before = tiles()
    got = mr.text_device(LENGTHS, args=[cuda_i64(lengths)])
    assert got.data_ptr() % 16 == lead
    assert got.cpu().numpy().tobytes() == b"".join(bytes([97 + i % 26]) * m for i, m in enumerate(lengths))
    assert routes_of(lengths).tolist() == [3, 1]
    assert (tiles() - before).tolist() == [3, 1]


@pytest.mark.gpu
def test_one_key_longer_than_the_stage_goes_direct_between_staged_tiles():
    mr = _mr("cuda")
    mr.map_device(41000, GEN_HOT)
    assert mr.collate() == 1001
    items = kmv_items(mr)
    assert sorted(len(v) for _, v in items) == [1] * 1000 + [40000]
    want = [ints_kmv(k, v) for k, v in items]
    before = tiles()
    assert text_of(mr, KMV_INTS) == b"".join(want)
    routes = routes_of([len(w) for w in want])
    assert routes.tolist() == [3, 1] and (tiles() - before).tolist() == [3, 1]
    assert mr.kmv.nkey == 1001 and kmv_items(mr) == items  # still the same KMV


# ---------------------------------------------------------------------- GPU: the KMV form

@pytest.mark.gpu
def test_kmv_form_with_1_2_and_257_variable_width_values():
    rng = np.random.default_rng(11)
    words = [b"", b"v", b"two", b"a longer value"]
    pairs = [(b"one", b"only")] + [(b"pair", b"first"), (b"pair", b"")]
    pairs += [(b"many-values", words[int(rng.integers(0, 4))]) for _ in range(257)]
    pairs += [(b"", b"under the empty key")]
    order = rng.permutation(len(pairs))
    mr = _host_mr([pairs[i] for i in order])
    assert mr.collate() == 4
    items = kmv_items(mr)
    assert sorted(len(v) for _, v in items) == [1, 1, 2, 257]
    assert {k: sorted(v) for k, v in items} == {k: sorted(v for kk, v in pairs if kk == k) for k, _ in pairs}
    assert text_of(mr, KMV_RAW) == b"".join(raw_kmv(k, v) for k, v in items)
    with pytest.raises(RuntimeError, match="mr_print"):  # the KV shape on a KMV
        mr.text_device(KV_RAW)


# ---------------------------------------------------------------------- GPU: bound buffers

@pytest.mark.gpu
def test_a_bound_table_and_new_contents_compile_once():
    n = 1000
    mr = _mr("cuda")
    mr.map_device(n, GEN)
    code = KV_ARGS + "// test_a_bound_table\n"  # a source no other test has compiled
    before = C.device_functor_compiles()
    tab = cuda_i64((np.arange(97) * 31 + 7) % 1009)
    for step in range(3):
        want = b"".join(b"%d\n" % v for v in tab.cpu().numpy()[np.arange(n) % tab.numel()])
        assert text_of(mr, code, args=[tab]) == want
        tab = cuda_i64(-(np.arange(50 + step) * 17 + step))  # new contents, a new tensor, another length
    assert C.device_functor_compiles() == before + 1
    assert mr.bound_device_args == []


# ---------------------------------------------------------------------- GPU: out of core

def _budget(mr, tmp_path):
    mr.hbm_budget = 128 << 10
    mr.host_budget = 1 << 20
    mr.memsize = -65536
    mr.fpath = str(tmp_path)


@pytest.mark.gpu
def test_kv_under_an_hbm_budget_equals_the_in_hbm_run(tmp_path):
    n = 50_000  # 800 000 bytes of pairs: pieces of a quarter of the budget
    ref = _mr("cuda")
    ref.map_device(n, GEN)
    want = text_of(ref, KV_LINE)
    assert want == b"".join(line_kv(i, struct.pack("<q", i * 7 + 1), struct.pack("<q", i * i)) for i in range(n))
    mr = _mr("cuda")
    _budget(mr, tmp_path)
    assert mr.map_device(n, GEN) == n
    assert not mr.kv.kdata.is_cuda  # host-resident: the op goes piece by piece
    assert text_of(mr, KV_LINE) == want  # index continues across the pieces
    f = str(tmp_path / "ooc.txt")
    assert mr.print_device(f, 0, -1, KV_LINE) == len(want)
    assert open(f, "rb").read() == want
    assert mr.kv.n == n and text_of(mr, KV_LINE) == want  # the data is still there


@pytest.mark.gpu
def test_kmv_under_an_hbm_budget(tmp_path):
    n = 40_000
    mr = _mr("cuda")
    _budget(mr, tmp_path)
    mr.map_device(n, GEN_GROUPS)
    assert mr.collate() == 3000
    got = text_of(mr, KMV_INTS)
    lines = got.split(b"\n")
    assert lines[-1] == b"" and len(lines) == 3001
    t = np.arange(n)
    want = {}
    for k, v in zip((t % 3000).tolist(), (t * 31 % 1009).tolist()):
        want.setdefault(k, []).append(v)
    for k, v in zip(((t[::2] // 2) % 3000).tolist(), (t[::2] % 17).tolist()):
        want.setdefault(k, []).append(v)
    have = {}
    for ln in lines[:-1]:
        k, vals = ln.split(b"\t")
        assert int(k) not in have
        have[int(k)] = sorted(int(x) for x in vals.split(b" "))
    assert have == {k: sorted(v) for k, v in want.items()}
    f = str(tmp_path / "ooc_kmv.txt")
    assert mr.print_device(f, 0, -1, KMV_INTS) == len(got)
    assert open(f, "rb").read() == got
    assert mr.kmv_parts >= 1 and text_of(mr, KMV_INTS) == got


# ---------------------------------------------------------------------- GPU: the op's contract

@pytest.mark.gpu
def test_print_device_file_and_rank_rules(tmp_path, capsys):
    n = 300
    mr = _mr("cuda")
    mr.map_device(n, GEN)
    items = kv_items(mr)
    want = b"".join(line_kv(i, k, v) for i, (k, v) in enumerate(items))
    f = str(tmp_path / "p.txt")
    assert mr.print_device(f, 0, -1, KV_LINE) == len(want) == os.path.getsize(f)
    assert open(f, "rb").read() == want
    os.remove(f)
    assert mr.print_device(f, 1, -1, KV_LINE) == len(want)  # fflag 1: file.<rank>
    assert open(f + ".0", "rb").read() == want and not os.path.exists(f)
    assert mr.print_device(f, 0, 0, KV_LINE) == len(want)  # proc 0: this rank
    assert open(f, "rb").read() == want
    os.remove(f)
    assert mr.print_device(f, 0, 1, KV_LINE) == 0  # proc 1: not this rank
    assert not os.path.exists(f)
    capsys.readouterr()
    assert mr.print_device(None, 0, -1, KV_LINE) == len(want)  # no file: the MR's output stream
    assert capsys.readouterr().out.encode() == want
    assert mr.kv.n == n and kv_items(mr) == items  # the pairs are as they were
    with pytest.raises(RuntimeError, match="has no mr_print"):
        mr.print_device(str(tmp_path / "q.txt"), 0, -1, GEN)
    assert not os.path.exists(str(tmp_path / "q.txt"))  # a functor that does not load opens no file
    with pytest.raises(RuntimeError, match="Could not open print file"):
        mr.print_device(str(tmp_path / "no" / "dir" / "q.txt"), 0, -1, KV_LINE)


# ---------------------------------------------------------------------- GPU: the other faces

def _rocm():
    from torch.utils.cpp_extension import ROCM_HOME
    return ROCM_HOME or os.environ.get("ROCM_PATH") or "/opt/rocm"


@pytest.mark.gpu
def test_capi_print_device(tmp_path):
    exe = str(tmp_path / "print_device_test")
    rocm = _rocm()
    subprocess.run(["gcc", "-O1", "-Wall", os.path.join(ROOT, "tests", "capi", "print_device_test.c"),
                    "-I", os.path.join(ROOT, "csrc", "capi"), "-L", PKG, "-lmrhip", f"-Wl,-rpath,{PKG}",
                    f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], check=True)
    (tmp_path / "gen.hip").write_text(GEN)
    (tmp_path / "print.hip").write_text(KV_LINE)
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = str(tmp_path / "c.txt")
    r = subprocess.run([exe, str(tmp_path / "gen.hip"), str(tmp_path / "print.hip"), out], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
    want = b"".join(line_kv(i, struct.pack("<q", i * 7 + 1), struct.pack("<q", i * i)) for i in range(1000))
    assert open(out, "rb").read() == want
    assert not os.path.exists(out + ".0")


@pytest.mark.gpu
def test_oink_print_device(tmp_path, monkeypatch):
    from gpu_mapreduce_amd.oink.interp import OINK, OinkError
    from gpu_mapreduce_amd.parallel.comm import Comm
    monkeypatch.chdir(tmp_path)
    o = OINK(Comm(device="cuda"), screen=io.StringIO(), logfile="log.oink")
    (tmp_path / "gen.hip").write_text(GEN)
    (tmp_path / "print.hip").write_text(KV_LINE)
    o.file(text="mr m\nm map/device 300 gen.hip\nm print/device oink.txt 0 -1 print.hip\n")
    want = b"".join(line_kv(i, struct.pack("<q", i * 7 + 1), struct.pack("<q", i * i)) for i in range(300))
    assert (tmp_path / "oink.txt").read_bytes() == want
    assert o.mr("m").kv.n == 300
    with pytest.raises(OinkError, match="Cannot open device functor file"):
        o.file(text="m print/device oink.txt 0 -1 no_such_file.hip\n")


def _html(rng, nlink, nurl=40):
    tag = b'<a href="'
    return b"".join(b"text " * int(rng.integers(0, 9)) + tag + b"http://h/%d" % int(rng.integers(0, nurl)) + b'">t</a>'
                    for _ in range(nlink))


@pytest.mark.gpu
def test_example_writes_the_index_from_file_names(tmp_path):
    import re
    rng = np.random.default_rng(5)
    contents = [_html(rng, 60), _html(rng, 45), _html(rng, 70)]
    names = []
    for i, data in enumerate(contents):
        names.append(str(tmp_path / f"page{i}.html"))
        with open(names[-1], "wb") as f:
            f.write(data)
    want = {}
    for name, data in zip(names, contents):
        for m in re.finditer(b'<a href="([^"]*)"', data):
            want.setdefault(m.group(1).decode(), set()).add(name)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = str(tmp_path / "index.txt")
    r = subprocess.run([sys.executable, EXAMPLE, out] + names, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(out, "rb").read().decode().splitlines()
    assert len(want) > 20 and len(lines) == len(want)
    # one line per URL, its files in file-list order, each once
    assert sorted(lines) == sorted(u + "\t" + " ".join(n for n in names if n in want[u]) for u in want)
    src = open(EXAMPLE).read()
    assert "scan_kv" not in src and "gather" not in src.split('"""', 2)[2]  # no host callback, nothing gathered


def test_example_module_loads_without_a_gpu():
    spec = importlib.util.spec_from_file_location("inverted_index_print_device", EXAMPLE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert C.device_print_check(mod.PRINT, True) > 0
    assert C.device_sortkey_check(mod.BY_FILE) > 0
    assert C.device_functor_check(mod.MAP, False) > 0
