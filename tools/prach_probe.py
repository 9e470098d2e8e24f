"""Times srs_amd_prach_detect_batch on the GPU: 64 occasions per call of (a) format 0, ZCZ 0, 4 ports and
(b) format B4, ZCZ 0, 30 kHz, 4 ports, all 64 preamble indices wanted (64 root sequences per occasion).

    PYTHONPATH=. python tools/prach_probe.py [--calls 200] [--warmup 20] [--occasions 64]

Device events around `--calls` back-to-back calls after warm-up (the roots are cached by then); prints one JSON line
per configuration with the time per call and per occasion.  The threshold and the margin do not change the work; the
values below are placeholders.  No test depends on these numbers (DESIGN.md records them with the machine named)."""
import argparse
import json
import sys

import numpy as np
import torch

import srsran_project_amd as amd


def occasion_words(rng, nof_elements):
    """Seeded unit-variance complex noise as cbf16 words."""
    x = (rng.standard_normal(nof_elements) + 1j * rng.standard_normal(nof_elements)) / np.sqrt(2.0)
    return amd.prach.to_cbf16(x).view(np.int16)


def run(det, name, cfg, nof_occasions, calls, warmup, device):
    g = amd.prach_geometry(cfg)
    rng = np.random.default_rng(7)
    sym = torch.from_numpy(np.concatenate([occasion_words(rng, g.nof_elements) for _ in range(nof_occasions)])).to(device)
    cfgs = amd.prach.PrachBatch([cfg] * nof_occasions)  # validated once: a cell's configuration is static
    results = torch.empty((nof_occasions, amd.prach.RESULT_BYTES), dtype=torch.uint8, device=device)
    for _ in range(warmup):
        det.detect_batch(sym, cfgs, results=results)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        det.detect_batch(sym, cfgs, results=results)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / calls
    print(json.dumps({"config": name, "occasions_per_call": nof_occasions, "calls": calls,
                      "workgroups_per_call": nof_occasions * g.nof_sequences, "idft_size": g.idft_size,
                      "us_per_call": round(ms * 1e3, 2), "us_per_occasion": round(ms * 1e3 / nof_occasions, 3),
                      "device": torch.cuda.get_device_name(device)}))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--occasions", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prach_probe needs a GPU")
    device = torch.device("cuda:0")
    det = amd.PrachDetector(0)
    F, S = amd.PrachFormat, amd.PrachSubcarrierSpacing
    run(det, "format0_zcz0_4ports", amd.PrachConfiguration(F.ZERO, S.KHZ1_25, 1, 0, threshold=0.053, win_margin=5,
                                                            nof_rx_ports=4), a.occasions, a.calls, a.warmup, device)
    run(det, "formatB4_zcz0_30khz_4ports", amd.PrachConfiguration(F.B4, S.KHZ30, 1, 0, threshold=0.081, win_margin=12,
                                                                   nof_rx_ports=4), a.occasions, a.calls, a.warmup,
        device)
    det.close()


if __name__ == "__main__":
    main()
