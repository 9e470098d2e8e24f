"""Times srs_amd_srs_estimate_batch on the GPU: 64 PDUs per call of (a) 4 antenna ports x 4 rx ports, M = 1632
(m_SRS 272, comb 2), one symbol and (b) 2 antenna ports x 4 rx ports, M = 144 (m_SRS 48, comb 4), four symbols.

    PYTHONPATH=. python tools/srs_probe.py [--calls 200] [--warmup 20] [--pdus 64] [--grids 8]

The PDUs of a call read `--grids` grids of 4 ports x 14 symbols x 3300 subcarriers in turn.  Device events around
`--calls` back-to-back calls after warm-up (the base sequences are cached by then); prints one JSON line per
configuration with the time per call and per PDU.  No test depends on these numbers (DESIGN.md records them with the
machine named)."""
import argparse
import json
import sys

import numpy as np
import torch

import srsran_project_amd as amd

NOF_PORTS, NOF_SUBC = 4, 3300


def to_cbf16(x):
    f = np.stack([np.real(x), np.imag(x)], axis=-1).astype(np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def run(est, name, cfg_kw, nof_pdus, nof_grids, calls, warmup, device):
    rng = np.random.default_rng(7)
    shape = (nof_grids, NOF_PORTS, 14, NOF_SUBC)
    grids = torch.from_numpy(to_cbf16((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0))
                             .view(np.int16)).to(device)
    batch = amd.SrsBatch([amd.SrsConfiguration(grid=i % nof_grids, **cfg_kw) for i in range(nof_pdus)])
    info = amd.srs_information(batch.configs[0])
    results = torch.empty((nof_pdus, amd.srs.RESULT_BYTES), dtype=torch.uint8, device=device)
    for _ in range(warmup):
        est.estimate_batch(grids, batch, results=results)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        est.estimate_batch(grids, batch, results=results)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / calls
    print(json.dumps({"config": name, "pdus_per_call": nof_pdus, "calls": calls,
                      "sequence_length": info.sequence_length, "idft_size": info.idft_size,
                      "us_per_call": round(ms * 1e3, 2), "us_per_pdu": round(ms * 1e3 / nof_pdus, 3),
                      "device": torch.cuda.get_device_name(device)}))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pdus", type=int, default=64)
    ap.add_argument("--grids", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("srs_probe needs a GPU")
    device = torch.device("cuda:0")
    est = amd.SrsEstimator(0)
    common = dict(sequence_id=1, bandwidth_index=0, comb_offset=0, cyclic_shift=0, numerology=1, rx_ports=[0, 1, 2, 3])
    run(est, "4x4_m1632_1symbol", dict(nof_antenna_ports=4, nof_symbols=1, start_symbol=13, configuration_index=61,
                                       comb_size=2, **common), a.pdus, a.grids, a.calls, a.warmup, device)
    run(est, "2x4_m144_4symbols", dict(nof_antenna_ports=2, nof_symbols=4, start_symbol=10, configuration_index=12,
                                       comb_size=4, **common), a.pdus, a.grids, a.calls, a.warmup, device)
    est.close()


if __name__ == "__main__":
    main()
