"""InvertedIndex (URL -> the files that link to it) from file names on, written
with device functors only: no host callback and no built-in text kernel
touches a byte of the files.

    python examples/python/inverted_index_device.py file.html [more files ...]

map_file_str_device splits the files at `<a href="`: every occurrence starts a
record, so a record holds one link and whatever follows it up to the next
link. The map functor scans its record to the closing quote and emits
(URL + NUL, int32 file index); collate groups the pairs by URL; the reduce
functor emits (URL + NUL, the int32 files of the URL). One output line per URL:
the URL, a tab, the files that link to it (sorted, each once).

(needs a GPU MapReduce; multi-GPU: torchrun --nproc-per-node 8 ...)"""
import struct
import sys

import gpu_mapreduce_amd as g

TAG = b'<a href="'
NMAP = 4     # chunks the files are split into; any number gives the same index
DELTA = 512  # look-ahead for a chunk boundary: more than the longest record start to the next tag may need

MAP = r"""
// one record = one link (the text before a file's first link is a record too:
// it does not start with the tag and emits nothing). A URL runs to the closing
// quote or, unclosed, to the end of its record; the key is the URL and a NUL,
// built in a local buffer: URLs longer than 255 bytes are cut there.
__device__ void mr_map(mrd::Bytes file, mrd::Bytes rec, long long offset, mrd::Emit& out) {
  const char tag[] = "<a href=\"";
  if (rec.n < 9) return;
  for (int i = 0; i < 9; ++i)
    if (rec.p[i] != (unsigned char)tag[i]) return;
  unsigned char url[256];
  int n = 0;
  while (9 + n < rec.n && rec.p[9 + n] != '"' && n < 255) {
    url[n] = rec.p[9 + n];
    ++n;
  }
  url[n] = 0;
  const int doc = (int)file.as<long long>();
  out.emit(url, n + 1, &doc, 4);
}
"""

REDUCE = r"""
// the values of a URL are its int32 file indices, contiguous: one record with all of them
__device__ void mr_reduce(mrd::Bytes url, mrd::Values files, mrd::Emit& out) {
  out.emit(url.p, url.n, files.d, 4 * files.n);
}
"""


def main():
    files = sys.argv[1:]
    if not files:
        print(__doc__)
        return 1
    comm = g.init()
    if not comm.is_cuda:
        print("device functors need a GPU MapReduce; nothing to do on the CPU engine")
        return 0
    mr = g.MapReduce(comm)
    nlinks = mr.map_file_str_device(NMAP, files, 0, 0, 0, TAG, DELTA, MAP)
    nurls = mr.collate()
    mr.reduce_device(REDUCE)
    mr.gather(1)
    index = {}

    def take(key, value):
        docs = struct.unpack(f"<{len(value) // 4}i", value)
        index[key[:-1].decode()] = sorted({files[d] for d in docs})

    mr.scan_kv(take)
    if comm.rank == 0:
        for url in sorted(index):
            print(url + "\t" + " ".join(index[url]))
        print(f"{nlinks} links, {nurls} URLs", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
