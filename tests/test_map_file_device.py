"""map_file_char_device / map_file_str_device: device functors over file
records (docs/api.md, "functors over file records").

Without a GPU: C.split_records on CPU tensors against the two Python oracles
of the record rules (char mode: `split` on the terminator; string mode: every
occurrence of the separator, overlapping ones included, starts a record), with
the 32 padding bytes filled so that reading padding as text completes a match;
C.device_text_check; the argument errors. On the GPU, one process: the split
kernels over the same cases against the oracle and the CPU twin, the two ops
end to end for nmap 1, 3 and 7, InvertedIndex parity with C.map_urls, the
compile count and the bound arguments, addflag, and the example script. Every
comparison is exact."""
import functools
import importlib.util
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_mapreduce_amd import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "examples", "python", "inverted_index_device.py")
TAG = b'<a href="'
PAD = 32

# ---------------------------------------------------------------------- sources

# (record bytes, {file, index})
RECORD = r"""
struct FI { long long file, index; };
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Emit& out) {
  const FI v{key.as<long long>(), index};
  out.emit(value.p, value.n, &v, 16);
}
"""
# the same with the bound buffers: (record length, table[file])
RECORD_ARGS = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Emit& out, const mrd::Args& args) {
  out.emit((long long)value.n, args[0].as<long long>()[key.as<long long>()]);
}
"""
TYPE_ERROR = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Emit& out) {
  out.emit(value.no_such_member, 1);
}
"""


# ---------------------------------------------------------------------- oracles

def oracle_char(data, n, c):
    """[(start, length)]: the rule of docs/api.md, char mode"""
    parts = data[:n].split(c)
    if parts[-1] == b"":
        parts.pop()
    recs, at = [], 0
    for p in parts:
        recs.append((at, len(p)))
        at += len(p) + 1
    return recs


def oracle_str(data, n, nread, sep):
    """[(start, length)]: the rule of docs/api.md, string mode"""
    if n == 0:
        return []
    m = [x.start() for x in re.finditer(b"(?=" + re.escape(sep) + b")", data[:nread]) if x.start() < n]
    starts = ([0] if not m or m[0] > 0 else []) + m
    ends = starts[1:] + [n]
    return list(zip(starts, (e - s for s, e in zip(starts, ends))))


def padded(data, nread, sep):
    """data[:nread] and 32 bytes of the separator's bytes, phased so that a
    separator cut off by nread is completed by the padding"""
    L = len(sep)
    return data[:nread] + (sep[L - 1:] + sep * (PAD + 1))[:PAD]


def _text(rng, n, alphabet):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).tolist())


def _put(buf, at, sep):
    b = bytearray(buf)
    b[at:at + len(sep)] = sep
    return bytes(b[:len(buf)]) if at + len(sep) <= len(buf) else bytes(b)


@functools.lru_cache(maxsize=None)
def cases():
    """(name, data, n, nread, sep, is_char); data has at least nread bytes"""
    rng = np.random.default_rng(20240607)
    out = []
    sizes = [0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5]
    seps = {1: b";", 2: b"ab", 9: TAG, 16: b"0123456789abcdef"}
    for n in sizes:
        out.append((f"char-random-{n}", _text(rng, n, b"abc\n\n"), n, n, b"\n", True))
        for L, sep in seps.items():
            d = bytearray(_text(rng, n + L - 1, b"xyz" + sep[:2]))
            for at in rng.integers(0, max(n, 1), size=max(1, n // 97)):
                if at + L <= len(d):
                    d[at:at + L] = sep
            d = bytes(d)
            out.append((f"str-L{L}-n{n}-tight", d, n, n, sep, False))
            out.append((f"str-L{L}-n{n}-ahead", d, n, n + L - 1, sep, False))
    n = 5000
    plain = b"x" * n
    for at in (0, n - 1, 15, 16, 4095, 4096):
        out.append((f"char-at-{at}", _put(plain, at, b"\n"), n, n, b"\n", True))
    both = plain
    for at in (0, 15, 16, 4095, 4096, n - 1):
        both = _put(both, at, b"\n")
    out.append(("char-all-places", both, n, n, b"\n", True))
    out.append(("char-adjacent", b"a\n\n\nb\n\n", 7, 7, b"\n", True))
    out.append(("char-all-terminators", b"\n" * 4100, 4100, 4100, b"\n", True))
    out.append(("char-no-terminator", b"q" * 4100, 4100, 4100, b"\n", True))
    out.append(("str-no-occurrence", b"q" * 4100, 4100, 4100, TAG, False))
    for L, sep in seps.items():
        if L > 1:
            out.append((f"str-L{L}-straddle-16", _put(plain, 16 - (L + 1) // 2, sep), n, n, sep, False))
            out.append((f"str-L{L}-straddle-4096", _put(plain, 4096 - (L + 1) // 2, sep), n, n, sep, False))
            out.append((f"str-L{L}-part-at-end", _put(plain, n - (L - 1), sep)[:n], n, n, sep, False))
        out.append((f"str-L{L}-ends-at-nread", _put(plain, n - L, sep), n, n, sep, False))
        out.append((f"str-L{L}-at-0", _put(plain, 0, sep), n, n, sep, False))
        # nread = n + L - 1: an occurrence that starts at n - 1 counts, one that starts at n does not
        d = b"x" * (n + L)
        out.append((f"str-L{L}-starts-at-n-1", _put(d, n - 1, sep), n, n + L - 1, sep, False))
        out.append((f"str-L{L}-starts-at-n", _put(d, n, sep), n, n + L - 1, sep, False))
    out.append(("str-aa-aaaaa", b"aaaaa", 5, 5, b"aa", False))
    out.append(("str-aa-runs", _text(rng, 9000, b"aab"), 9000, 9000, b"aa", False))
    out.append(("str-aa-all-a", b"a" * 4200, 4199, 4200, b"aa", False))
    return out


def expected(case):
    _, data, n, nread, sep, is_char = case
    return oracle_char(data, n, sep) if is_char else oracle_str(data, n, nread, sep)


def records_of(off, nrec, is_char):
    o = off.cpu().numpy()
    assert o.dtype == np.int64 and o.shape == (nrec + 1,)
    trim = 1 if is_char else 0
    return [(int(o[i]), int(o[i + 1] - trim - o[i])) for i in range(nrec)]


def split(case, device):
    _, data, n, nread, sep, is_char = case
    text = torch.tensor(list(padded(data, nread, sep)), dtype=torch.uint8).to(device)
    off, nrec = C.split_records(text, n, nread, sep, is_char)
    assert off.device == text.device
    return off, nrec


def _mr(device):
    from gpu_mapreduce_amd.parallel.comm import Comm
    from gpu_mapreduce_amd.runtime.mapreduce import MapReduce
    return MapReduce(Comm(device=device))


# ---------------------------------------------------------------------- no GPU

def test_oracles_on_the_examples_of_the_rules():
    assert oracle_str(b"aaaaa", 5, 5, b"aa") == [(0, 1), (1, 1), (2, 1), (3, 2)]
    assert oracle_char(b"a\n\nb", 4, b"\n") == [(0, 1), (2, 0), (3, 1)]
    assert oracle_char(b"a\n", 2, b"\n") == [(0, 1)] and oracle_char(b"", 0, b"\n") == []
    assert oracle_str(b"xx<a", 4, 4, b"<a") == [(0, 2), (2, 2)] and oracle_str(b"xx", 2, 2, b"<a") == [(0, 2)]


def test_split_records_cpu_equals_the_oracles():
    for case in cases():
        off, nrec = split(case, "cpu")
        assert records_of(off, nrec, case[5]) == expected(case), case[0]


def test_split_records_argument_errors():
    text = torch.zeros(64 + PAD, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="0 bytes; it must have 1 to 16 bytes"):
        C.split_records(text, 64, 64, b"", False)
    with pytest.raises(RuntimeError, match="17 bytes; it must have 1 to 16 bytes"):
        C.split_records(text, 64, 64, b"x" * 17, False)
    with pytest.raises(RuntimeError, match="padded by >= 32 bytes"):
        C.split_records(text, 64, 65, b"x", False)
    with pytest.raises(RuntimeError, match="terminator"):
        C.split_records(text, 64, 64, b"xy", True)


def test_device_text_check():
    before = C.device_functor_compiles()
    assert C.device_text_check(RECORD) > 0
    assert C.device_text_check(RECORD_ARGS) > 0
    with pytest.raises(RuntimeError, match="does not compile") as e:
        C.device_text_check(TYPE_ERROR)
    assert "no_such_member" in str(e.value)
    assert C.device_functor_compiles() == before + 3


def test_ops_need_a_gpu_mapreduce_and_a_separator_within_the_limit(tmp_path):
    f = tmp_path / "a.txt"
    f.write_bytes(b"one\ntwo\n")
    mr = _mr("cpu")
    with pytest.raises(RuntimeError, match=r"device functors run on a GPU MapReduce \(device cuda\)"):
        mr.map_file_char_device(1, [str(f)], 0, 0, 0, b"\n", 16, RECORD)
    with pytest.raises(RuntimeError, match=r"device functors run on a GPU MapReduce \(device cuda\)"):
        mr.map_file_str_device(1, [str(f)], 0, 0, 0, b"tw", 16, RECORD)
    with pytest.raises(RuntimeError, match="separator of 1 to 16 bytes, 0 given"):
        mr.map_file_str_device(1, [str(f)], 0, 0, 0, b"", 16, RECORD)
    with pytest.raises(RuntimeError, match="separator of 1 to 16 bytes, 17 given"):
        mr.map_file_str_device(1, [str(f)], 0, 0, 0, b"s" * 17, 16, RECORD)


# ---------------------------------------------------------------------- GPU

def kv_pairs(kv):
    """the pairs of a native KV as [(key bytes, value bytes)]"""
    if kv is None or kv.n == 0:
        return []

    def col(data, off, w):
        d = data.cpu().numpy().tobytes()
        if w >= 0:
            return [d[i * w:(i + 1) * w] for i in range(kv.n)]
        o = off.cpu().numpy()
        return [d[o[i]:o[i + 1]] for i in range(kv.n)]

    return list(zip(col(kv.kdata, kv.koff, kv.kw), col(kv.vdata, kv.voff, kv.vw)))


def pairs_of(mr):
    return kv_pairs(mr.kv)


def file_records(files, recs_of):
    """sorted [(record bytes, pack(file, index))] of the files' contents"""
    out = []
    for i, data in enumerate(files):
        out += [(data[s:s + ln], struct.pack("<qq", i, s)) for s, ln in recs_of(data)]
    return sorted(out)


def write_files(tmp_path, contents):
    names = []
    for i, c in enumerate(contents):
        p = tmp_path / f"f{i}.txt"
        p.write_bytes(c)
        names.append(str(p))
    return names


@pytest.mark.gpu
def test_split_records_gpu_equals_the_oracles_and_the_cpu_twin():
    for case in cases():
        off, nrec = split(case, "cuda:0")
        coff, cnrec = split(case, "cpu")
        assert records_of(off, nrec, case[5]) == expected(case), case[0]
        assert nrec == cnrec and torch.equal(off.cpu(), coff), case[0]


def _lines_file():
    rng = np.random.default_rng(7)
    lines, size = [], 0
    while size < 10 * 1024:
        ln = b"" if rng.integers(0, 6) == 0 else _text(rng, int(rng.integers(1, 90)), b"abcdefgh ")
        if size < 4096 <= size + 150 and size + len(ln) + 1 <= 4096:
            ln = b"L" * 150  # the line that crosses byte 4096
        lines.append(ln)
        size += len(ln) + 1
    data = b"\n".join(lines) + b"\n"
    at = data.index(b"L" * 150)
    assert at < 4096 < at + 150 and b"\n\n" in data
    return data


@pytest.mark.gpu
def test_map_file_char_device_end_to_end(tmp_path):
    contents = [b"", b"first\n\nlast without a newline", _lines_file()]
    names = write_files(tmp_path, contents)
    want = file_records(contents, lambda d: oracle_char(d, len(d), b"\n") if d else [])
    assert any(k == b"" for k, _ in want)
    for nmap in (1, 3, 7):
        mr = _mr("cuda:0")
        n = mr.map_file_char_device(nmap, names, 0, 0, 0, b"\n", 256, RECORD)
        assert mr.mapfilecount == 3
        assert n == len(want) and sorted(pairs_of(mr)) == want, nmap


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["aa", "href"])
def test_map_file_str_device_end_to_end(tmp_path, which):
    rng = np.random.default_rng(11)
    if which == "aa":
        sep, delta = b"aa", 64
        contents = [b"", _text(rng, 6000, b"aab"), b"baaab"]
    else:
        sep, delta = TAG, 512
        body = b"".join(_text(rng, int(rng.integers(0, 60)), b"<a hrefxyz \n") + TAG + _text(rng, 12, b"uvw/.") + b'">t</a>'
                        for _ in range(150))
        contents = [b"no link here", body, TAG + b'only">']
    names = write_files(tmp_path, contents)
    want = file_records(contents, lambda d: oracle_str(d, len(d), len(d), sep))
    for nmap in (1, 3, 7):
        mr = _mr("cuda:0")
        n = mr.map_file_str_device(nmap, names, 0, 0, 0, sep, delta, RECORD)
        assert n == len(want) and sorted(pairs_of(mr)) == want, nmap


def _example():
    spec = importlib.util.spec_from_file_location("inverted_index_device", EXAMPLE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _html(rng, nlink, nurl=40):
    """links whose URL is closed by a quote and holds no '<'"""
    return b"".join(_text(rng, int(rng.integers(0, 50)), b"<a href xyz\n") + TAG + b"http://h/%d" % int(rng.integers(0, nurl)) + b'">t</a>'
                    for _ in range(nlink))


@pytest.mark.gpu
def test_inverted_index_functor_equals_map_urls():
    """Every URL of this text is closed by a quote and holds no '<': the
    functor's scan, bounded by its record, and map_urls' scan, bounded by the
    text alone, then see the same bytes. That is the only kind of text on
    which the two agree (an unclosed URL ends with its record for the functor
    and runs on for map_urls)."""
    data = _html(np.random.default_rng(3), 300) + b"tail"
    n, doc = len(data), 5
    text = torch.tensor(list(data + bytes(PAD)), dtype=torch.uint8).cuda()
    off, nrec = C.split_records(text, n, n, TAG, False)
    got = C.device_map_records(text, off, nrec, 0, doc, 0, _example().MAP)
    ref = C.map_urls(text, n, doc)
    assert ref.n == 300 and got.vw == 4
    assert sorted(kv_pairs(got)) == sorted(kv_pairs(ref))
    assert all(k.endswith(b"\0") and v == struct.pack("<i", doc) for k, v in kv_pairs(got))


@pytest.mark.gpu
def test_one_compile_for_new_files_and_nmap_and_bound_arguments(tmp_path):
    a = write_files(tmp_path, [b"x\nyy\n", b"zzz\n"])
    (tmp_path / "more").mkdir()
    b = write_files(tmp_path / "more", [_lines_file()])
    src = RECORD_ARGS + "// test_one_compile\n"  # a source no other test has compiled
    table, prev = torch.tensor([100, 200], dtype=torch.int64).cuda(), torch.zeros(1, dtype=torch.int64).cuda()
    mr = _mr("cuda:0")
    mr.device_args(prev)
    before = C.device_functor_compiles()
    assert mr.map_file_char_device(2, a, 0, 0, 0, b"\n", 4, src, args=[table]) == 3
    got = sorted((struct.unpack("<q", k)[0], struct.unpack("<q", v)[0]) for k, v in pairs_of(mr))
    assert got == [(1, 100), (2, 100), (3, 200)]
    bound = mr.bound_device_args
    assert len(bound) == 1 and bound[0].data_ptr() == prev.data_ptr()
    data = _lines_file()
    assert mr.map_file_char_device(5, b, 0, 0, 0, b"\n", 256, src, args=[table]) == len(oracle_char(data, len(data), b"\n"))
    # the other mode (the newline starts a record)
    assert mr.map_file_str_device(3, b, 0, 0, 0, b"\n", 256, src, args=[table]) == len(oracle_str(data, len(data), len(data), b"\n"))
    assert C.device_functor_compiles() == before + 1


@pytest.mark.gpu
def test_addflag_appends_and_returns_the_total(tmp_path):
    names = write_files(tmp_path, [b"a\nb\nc\n", b"d\ne"])
    mr = _mr("cuda:0")
    assert mr.map_file_char_device(1, names[:1], 0, 0, 0, b"\n", 4, RECORD) == 3
    first = pairs_of(mr)
    assert mr.map_file_char_device(1, names[1:], 0, 0, 0, b"\n", 4, RECORD, addflag=1) == 5
    assert pairs_of(mr)[:3] == first
    assert sorted(k for k, _ in pairs_of(mr)) == [b"a", b"b", b"c", b"d", b"e"]
    assert mr.map_file_char_device(1, names[1:], 0, 0, 0, b"\n", 4, RECORD) == 2


@pytest.mark.gpu
def test_example_script_prints_the_index(tmp_path):
    rng = np.random.default_rng(5)
    contents = [_html(rng, 60), _html(rng, 45), b"nothing", _html(rng, 70)]
    names = write_files(tmp_path, contents)
    want = {}
    for name, data in zip(names, contents):
        for m in re.finditer(re.escape(TAG) + b'([^"]*)"', data):
            want.setdefault(m.group(1).decode(), set()).add(name)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, EXAMPLE] + names, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        url, files = line.split("\t")
        got[url] = set(files.split(" "))
    assert len(want) > 20 and got == want
    assert r.stdout.splitlines() == [u + "\t" + " ".join(sorted(want[u])) for u in sorted(want)]
