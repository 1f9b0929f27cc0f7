"""The stream hand-off of a spool's pieces (csrc/engine/streams.h, spool.h).

`C.spool_upload` is one step of the out-of-core convert pipeline: pieces are
added to a fresh Spool on the current stream, ooc.h's upload_spool copies them
into one device KV on a pool side stream, and the current stream takes the
result over — the calls the loop in ooc_convert_parts makes.

* CPU: the same code without streams returns the concatenation.
* GPU: pieces whose contents are still being written by the current stream
  when the upload is queued must arrive complete: Spool::take() orders the side
  stream behind the stream that added the HBM-tier pieces and marks them as
  used there, so they may be dropped right after."""
import time

import pytest
import torch

import gpu_mapreduce_amd as g

C = g._ext.C


def _pairs(kv):
    out = []
    C.kv_iter(kv, lambda i, k, v: out.append((bytes(k), bytes(v))))
    return out


def _fixed(n, base):
    k = torch.arange(base, base + n, dtype=torch.int64)
    kv = C.make_kv(k.view(torch.uint8), None, (k * 3 + 1).view(torch.uint8), None, n, "cpu")
    kv.kw = kv.vw = 8  # (make_kv cannot tell the widths of an empty piece)
    return kv


def _var(n, base):
    keys = [b"k%d" % (base + i) * (1 + (base + i) % 3) for i in range(n)]
    vals = [b"v" * ((base + i) % 5) for i in range(n)]
    off = lambda xs: torch.tensor([0] + [sum(map(len, xs[:i + 1])) for i in range(len(xs))], dtype=torch.int64)
    data = lambda xs: torch.tensor(list(b"".join(xs)), dtype=torch.uint8)
    return C.make_kv(data(keys), off(keys), data(vals), off(vals), n, "cpu")


@pytest.mark.parametrize("make", [_fixed, _var], ids=["fixed8", "variable"])
def test_upload_is_the_concatenation_cpu(make):
    pieces = [make(1, 0), make(1000, 1), make(0, 1001)]
    want = [p for kv in pieces for p in _pairs(kv)]
    got = C.spool_upload(pieces, "cpu")
    assert got.n == 1001
    assert _pairs(got) == want


# Main-stream work queued in front of the pieces' last write: NSORT sorts of
# 2^26 int64. Measured on an MI355X: the sorts keep the device busy for 47 ms
# and spool_upload has returned 6 ms after the first was launched (with 2^24
# elements: 13 ms against 7 ms, too close).
NSORT = 8


@pytest.mark.gpu
def test_upload_waits_for_the_stream_that_wrote_the_pieces():
    dev = "cuda:0"
    n = 1 << 16

    def piece():
        k = torch.zeros(n, dtype=torch.int64, device=dev)
        v = torch.zeros(n, dtype=torch.int64, device=dev)
        return k, v, C.make_kv(k.view(torch.uint8), None, v.view(torch.uint8), None, n, dev)

    junk = torch.randint(0, 1 << 60, (1 << 26,), dtype=torch.int64, device=dev)
    # warm up what the timed part uses (sort workspace, the stream pool, the copy kernels)
    junk.sort()
    C.spool_upload([piece()[2]], dev)
    pieces = [piece(), piece()]
    torch.cuda.synchronize()

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    h0 = time.perf_counter()
    for _ in range(NSORT):
        junk.sort()
    t1.record()
    for p in pieces:  # the last write of the pieces, behind the delay
        p[0].fill_(7)
        p[1].fill_(7)
    out = C.spool_upload([p[2] for p in pieces], dev)
    # the upload was queued while the pieces were still unwritten, or this test shows nothing
    assert not t1.query(), "delay too short"
    call_ms = 1e3 * (time.perf_counter() - h0)
    del pieces, p
    # the pieces' blocks are free now: whoever gets them next must not disturb the upload
    again = [torch.empty(n, dtype=torch.int64, device=dev).fill_(9) for _ in range(4)]
    torch.cuda.synchronize()
    print(f"delay {t0.elapsed_time(t1):.1f} ms on the device, upload queued {call_ms:.1f} ms after its start")
    assert out.n == 2 * n
    assert bool((out.kdata.view(torch.int64) == 7).all()) and bool((out.vdata.view(torch.int64) == 7).all())
    assert all(bool((a == 9).all()) for a in again)
