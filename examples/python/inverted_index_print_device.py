"""InvertedIndex (URL -> the files that link to it) from file names to an output
file with device functors only: no host callback touches a byte of the files
or of the index, and nothing is gathered.

    python examples/python/inverted_index_print_device.py index.txt file.html [more files ...]

The map and the collate are those of inverted_index_device.py: map_file_str_
device splits the files at `<a href="`, the map functor emits (URL + NUL, int32
file index), collate groups the pairs by URL. Then sort_multivalues_device
orders every URL's file indices (a sort-key functor on the int32), and
print_device formats the KMV on the GPU: the print functor takes the KMV form
of mr_print and the file names as two bound buffers (their bytes, and int64
offsets), and writes one line per URL: the URL, a tab, the names of the files
that link to it (in file-list order, each once), a newline. The lines come in
the KMV's key order; with several ranks every rank's lines follow the previous
rank's.

(needs a GPU MapReduce)"""
import sys

import numpy as np
import torch

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

BY_FILE = r"""
// a URL's values are int32 file indices (never negative): their own order
__device__ unsigned long long mr_sortkey(mrd::Bytes v) { return (unsigned long long)v.as<int>(); }
"""

PRINT = r"""
// args[0] = the file names, back to back; args[1] = int64 offsets, one more than names.
// The values are sorted: a file that links to the URL twice is two neighbours.
__device__ void mr_print(mrd::Bytes url, mrd::Values files, mrd::Text& out, const mrd::Args& args) {
  const unsigned char* names = args[0].as<unsigned char>();
  const long long* at = args[1].as<long long>();
  out.put(url.p, url.n - 1);  // without the NUL
  out.chr('\t');
  int prev = -1;
  for (long long i = 0; i < files.n; ++i) {
    const int f = files.get<int>(i);
    if (f == prev) continue;
    if (prev >= 0) out.chr(' ');
    out.put(names + at[f], at[f + 1] - at[f]);
    prev = f;
  }
  out.chr('\n');
}
"""


def main():
    if len(sys.argv) < 3:
        print(__doc__)
        return 1
    path, files = sys.argv[1], sys.argv[2:]
    comm = g.init()
    if not comm.is_cuda:
        print("device functors need a GPU MapReduce; nothing to do on the CPU engine")
        return 0
    mr = g.MapReduce(comm)
    nlinks = mr.map_file_str_device(NMAP, files, 0, 0, 0, TAG, DELTA, MAP)
    nurls = mr.collate()
    mr.sort_multivalues_device(BY_FILE, bits=32)
    raw = [f.encode() for f in files]
    names = torch.from_numpy(np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy()).to(mr.device)
    at = torch.from_numpy(np.cumsum([0] + [len(r) for r in raw], dtype=np.int64)).to(mr.device)
    nbytes = mr.print_device(path, 0, -1, PRINT, args=[names, at])
    if comm.rank == 0:
        print(f"{nlinks} links, {nurls} URLs, {nbytes} bytes to {path}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
