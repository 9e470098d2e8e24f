"""The 64-cell PDSCH encode stage alone: HIP-event time of encode_batch on one warm stream (20 calls).  Run under
rocprofv3 --kernel-trace --stats for the kernels' own durations.  PYTHONPATH=. python tools/pdsch_stage_probe.py"""
import torch

import bench_pipeline as bp

dev = torch.device("cuda", 0)
pl = bp.Pipeline(64, dev)
s = torch.cuda.Stream(dev)
for _ in range(3):
    pl.enc.encode_batch(pl.tb_dl, pl.plan_dl, out=pl.cw_dl, stream=s)
torch.cuda.synchronize(dev)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(s)
for _ in range(20):
    pl.enc.encode_batch(pl.tb_dl, pl.plan_dl, out=pl.cw_dl, stream=s)
e1.record(s)
torch.cuda.synchronize(dev)
print("%.4f ms per encode_batch (64 TBs, 8256 codeblocks)" % (e0.elapsed_time(e1) / 20))
