"""Writes tests/golden/inflate/libdeflate_streams.json.gz: raw DEFLATE streams from libdeflate's encoder (what htslib, and so most BAMs in the field, are
written with), for tests/test_emu_inflate_corners.py and tests/test_gpu_inflate_corners.py.  Needs libdeflate.so.0 on the machine (loaded through ctypes; nothing
is fetched).  The fixture keeps the compressed streams and their names only: the tests take the expected bytes from zlib's decode of each stream.

    python tools/make_inflate_fixtures.py"""
import base64
import ctypes
import gzip
import json
import os
import sys
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
OUT = os.path.join(REPO, "tests", "golden", "inflate", "libdeflate_streams.json.gz")
LEVELS = (0, 1, 6, 9, 12)
CUTS = (1, 17, 300)
MAX_PAYLOAD = 8192


def main():
    try:
        ld = ctypes.CDLL("libdeflate.so.0")
    except OSError as e:
        sys.exit("libdeflate.so.0 is not on this machine (%s): the fixture cannot be made here" % e)
    ld.libdeflate_alloc_compressor.restype = ctypes.c_void_p; ld.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    ld.libdeflate_free_compressor.restype = None; ld.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    ld.libdeflate_deflate_compress_bound.restype = ctypes.c_size_t; ld.libdeflate_deflate_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    ld.libdeflate_deflate_compress.restype = ctypes.c_size_t
    ld.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]

    def deflate(data, level):
        c = ld.libdeflate_alloc_compressor(level)
        assert c, "libdeflate has no level %d" % level
        try:
            cap = ld.libdeflate_deflate_compress_bound(c, len(data))
            buf = ctypes.create_string_buffer(cap)
            n = ld.libdeflate_deflate_compress(c, data, len(data), buf, cap)
            assert n > 0
            return buf.raw[:n]
        finally:
            ld.libdeflate_free_compressor(c)

    from test_emu_inflate import payloads
    streams = []
    for kind, data in payloads(np.random.default_rng(5)).items():
        data = data[:MAX_PAYLOAD]
        for level in LEVELS:
            streams.append(("%s_level%d" % (kind, level), data, level))
        for cut in CUTS:
            streams.append(("%s_cut%d" % (kind, cut), data[:cut], 6))
    doc = {"encoder": "libdeflate (libdeflate_deflate_compress)", "streams": []}
    for name, data, level in streams:
        s = deflate(data, level)
        assert zlib.decompress(s, -15) == data, name
        doc["streams"].append({"name": name, "deflate": base64.b64encode(s).decode()})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(doc, indent=0).encode())
    print("%s: %d streams, %d bytes" % (OUT, len(streams), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
