#!/usr/bin/env python3
"""Host cost of a small K_map submission: wall time of phz_map_reads_batch on ONE resident shard of ~1,500 read pairs (a handful of tiles: the kernels are
done in microseconds, what is left is launch_map_batch itself -- table image, reservations, five launches, the read-back and the host wait).
  tools/map_submit_time.py [calls=1000] [pairs=1500]      -> one line: median / p10 / p90 in us, calls per submission
PHZ_LIB_PATH=<another libphz.so> times another build of the library under the same Python."""
import os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
import torch
from phaser_amd import soa, synth
from phaser_amd.mapper import Mapper

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 1500
v, gs, ge, w = synth.make_variants("chr1", 1, 30_000_000, 400, 702, n_genes=16)
rb = synth.make_reads(v, gs, ge, w, pairs, 802, n_rate=0.002)
rb = rb.select(synth.samtools_keep(rb, 255))
shard = soa.pack_readbatch(rb).to("cuda:0")
m = Mapper(0)
first = m.map_batch([shard], [v.pos], 10)
call, bufs, N = m.prepare_batch([shard], [v.pos], 10, [first[0].n + 16], aux=False)
for _ in range(50):
    m.ctx.check(call())
torch.cuda.synchronize()
t = []
for _ in range(calls):
    t0 = time.perf_counter()
    st = call()
    t.append(time.perf_counter() - t0)
    m.ctx.check(st)
assert int(N[0]) == first[0].n
t.sort()
print("map_submit_time: %d records, %d calls per submission, %d submissions: median %.2f us, p10 %.2f, p90 %.2f"
      % (shard.n, first[0].n, calls, t[len(t) // 2] * 1e6, t[len(t) // 10] * 1e6, t[9 * len(t) // 10] * 1e6))
