"""Times srs_amd_prach_demodulate_batch on the GPU: 64 windows per call at 122.88 MHz of (a) format 0, 30 kHz PUSCH,
273 PRB, 4 ports (one 98304-point symbol per port: the split path, 96 x 1024) and (b) format B4, 30 kHz, 4 ports, one
time-domain occasion (twelve 4096-point symbols per port: the planned path), and each followed by the detector on the
same stream (srs_amd_prach_detect_batch on the demodulator's output, no host copy between them).

    PYTHONPATH=. python tools/prach_demod_probe.py [--calls 50] [--warmup 5] [--windows 64]

Device events around `--calls` back-to-back calls after warm-up; prints one JSON line per configuration with the time
per call, the bytes the launch must read (8 x N x symbols x ports x windows) and the share of the HBM bandwidth that
rate is (of the 6.3 TB/s a streaming copy achieves on this part, and of the 8 TB/s specification).  The windows of a
call are distinct buffers, 250 MB (a) / 100 MB (b) in all, so the samples come from HBM and not from a cache.  No test
depends on these numbers (DESIGN.md records them with the machine named)."""
import argparse
import json
import sys

import torch

import srsran_project_amd as amd

SRATE = 122880000
ACHIEVABLE_TBS, SPEC_TBS = 6.3, 8.0


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls * 1e3  # microseconds per call


def run(dem, det, name, cfg, pcfg, nof_windows, calls, warmup, device):
    g = dem.geometry(cfg)
    n = g.window_samples
    gen = torch.Generator(device=device).manual_seed(7)
    samples = torch.randn((nof_windows, cfg.nof_ports, n, 2), generator=gen, device=device, dtype=torch.float32)
    cfgs = [cfg] * nof_windows
    s_off = [i * cfg.nof_ports * n for i in range(nof_windows)]
    o_off = dem.packed_offsets(cfgs)
    out = torch.empty(nof_windows * g.nof_elements, dtype=torch.int32, device=device)
    pbatch = amd.prach.PrachBatch([pcfg] * (nof_windows * cfg.nof_td_occasions * cfg.nof_fd_occasions),
                                  dem.detector_offsets(cfgs, o_off))
    results = torch.empty((pbatch.n, amd.prach.RESULT_BYTES), dtype=torch.uint8, device=device)

    batch = amd.PrachDemodBatch(SRATE, cfgs, s_off, [n] * nof_windows, out_offsets=o_off)  # validated once

    def demod():
        dem.demodulate_batch(samples, batch, out=out)

    def chain():
        demod()
        det.detect_batch(out, pbatch, results=results)

    us = timed(demod, calls, warmup)
    us_chain = timed(chain, calls, warmup)
    read = 8 * g.dft_size * g.nof_symbols * cfg.nof_td_occasions * cfg.nof_ports * nof_windows
    tbs = read / us * 1e-6
    print(json.dumps({"config": name, "windows_per_call": nof_windows, "calls": calls, "dft_size": g.dft_size,
                      "sub_dft_size": g.sub_dft_size, "nof_sub_dfts": g.nof_sub_dfts,
                      "us_per_call": round(us, 1), "us_per_window": round(us / nof_windows, 2),
                      "bytes_read": read, "tb_per_s": round(tbs, 3),
                      "share_of_achievable_6.3": round(tbs / ACHIEVABLE_TBS, 3),
                      "share_of_spec_8.0": round(tbs / SPEC_TBS, 3),
                      "us_per_call_with_detector": round(us_chain, 1),
                      "device": torch.cuda.get_device_name(device)}))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prach_demod_probe needs a GPU")
    device = torch.device("cuda:0")
    dem, det = amd.PrachDemodulator(SRATE, 0), amd.PrachDetector(0)
    F, S = amd.PrachFormat, amd.PrachSubcarrierSpacing
    run(dem, det, "format0_122.88MHz_4ports",
        amd.PrachDemodConfiguration(F.ZERO, numerology=1, nof_prb_ul_grid=273, rb_offset=100, nof_ports=4),
        amd.PrachConfiguration(F.ZERO, S.KHZ1_25, 1, 0, threshold=0.053, win_margin=5, nof_rx_ports=4),
        a.windows, a.calls, a.warmup, device)
    run(dem, det, "formatB4_30khz_122.88MHz_4ports",
        amd.PrachDemodConfiguration(F.B4, numerology=1, nof_prb_ul_grid=273, rb_offset=100, nof_ports=4),
        amd.PrachConfiguration(F.B4, S.KHZ30, 1, 0, threshold=0.081, win_margin=12, nof_rx_ports=4),
        a.windows, a.calls, a.warmup, device)
    det.close()
    dem.close()


if __name__ == "__main__":
    main()
