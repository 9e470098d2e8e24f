"""Times srs_amd_csi_rs_map_slot on the GPU: a TRS slot per cell (two row-1 resources at l0 = 4 and 8) plus one
row-4 resource at l0 = 13, all on 273 PRB, for (a) 64 cells' grids in one call and (b) one grid.

    PYTHONPATH=. python tools/csi_rs_probe.py [--calls 500] [--warmup 50] [--repeats 7] [--grids 64]

Grids are 4 ports x 14 symbols x 3276 subcarriers.  Device events around `--calls` back-to-back calls after warm-up,
`--repeats` such windows per configuration, the two configurations alternating; prints one JSON line per
configuration with the median and the spread (min, max) of the time per call and per resource.  No test depends on
these numbers (DESIGN.md records them beside the reference's ref_map_us of tests/golden/csi_rs_golden.npz)."""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

import srsran_project_amd as amd

NOF_PORTS, NOF_SUBC, NOF_RB = 4, 3276, 273


def resources(nof_grids):
    out = []
    for g in range(nof_grids):
        for l0 in (4, 8):
            out.append(amd.CsiRsConfig(row=1, k_ref=[0], symbol_l0=l0, start_rb=0, nof_rb=NOF_RB,
                                       cdm=amd.csi_rs.CDM_NONE, freq_density=amd.csi_rs.DENSITY_THREE,
                                       scrambling_id=g % 1024, slot_index=3, grid=g))
        out.append(amd.CsiRsConfig(row=4, k_ref=[4], symbol_l0=13, start_rb=0, nof_rb=NOF_RB, cdm=amd.csi_rs.CDM_FD2,
                                   freq_density=amd.csi_rs.DENSITY_ONE, scrambling_id=(g + 500) % 1024, slot_index=3,
                                   grid=g))
    return out


def window(gen, grids, cfgs, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        gen.map_slot(grids, cfgs)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--grids", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("csi_rs_probe needs a GPU")
    device = torch.device("cuda:0")
    gen = amd.CsiRsGenerator(0)
    setups = {}
    for name, n in (("%d_grids" % a.grids, a.grids), ("1_grid", 1)):
        grids = torch.zeros((n, NOF_PORTS, 14, NOF_SUBC, 2), dtype=torch.int16, device=device)
        cfgs = amd.CsiRsBatch(resources(n))
        for _ in range(a.warmup):
            gen.map_slot(grids, cfgs)
        setups[name] = (grids, cfgs, [])
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, (grids, cfgs, times) in setups.items():
            times.append(window(gen, grids, cfgs, a.calls))
    for name, (grids, cfgs, times) in setups.items():
        med = statistics.median(times)
        print(json.dumps({"config": name, "resources_per_call": cfgs.n, "calls": a.calls, "repeats": a.repeats,
                          "us_per_call_median": round(med, 2), "us_per_call_min": round(min(times), 2),
                          "us_per_call_max": round(max(times), 2),
                          "us_per_resource_median": round(med / cfgs.n, 3),
                          "device": torch.cuda.get_device_name(device)}))
        sys.stdout.flush()
    gen.close()


if __name__ == "__main__":
    main()
