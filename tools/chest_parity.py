"""Parity table of the PUSCH channel estimator on the coherent edge cases (tests/chest_cases.EDGE_CASES): per
case the share of estimate words that are not bit-identical -- GPU vs oracle and reference vs oracle, over the whole
buffer and over the allocation's edge band --, the largest relative difference of an estimate, and the six
statistics of port 0 from the GPU, the oracle and the reference.  Shows how far inside the 1e-3 share cap and the
2e-3 statistic tolerance of tests/test_pusch_chest_gpu.py the kernel sits.

  python tools/chest_parity.py [output.md]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from oracle import chest  # noqa: E402
from tests import chest_cases as cc  # noqa: E402

KEYS = ["noise_var", "epre", "rsrp", "snr", "time_alignment_s", "cfo_hz"]


def max_rel(a, b):
    x, y = cc.to_cf(a), cc.to_cf(b)
    with np.errstate(all="ignore"):
        r = np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-30)
    r = r[np.asarray(a, np.uint32) != np.asarray(b, np.uint32)]
    return float(r.max()) if r.size else 0.0


def share(a, b, where=None):
    bad, n = cc.share_differing(a, b, where)
    return "%d / %d (%.1e)" % (bad, n, bad / n)


def main():
    import srsran_project_amd as amd

    est = amd.DmrsPuschEstimator(device=0)
    out = ["# PUSCH channel estimator on coherent DM-RS: GPU vs oracle vs reference", "",
           "Differing estimate words (count / words looked at (share)); cap 1e-3 of the whole buffer, and of the edge",
           "band (first and last 24 REs of the allocation in every written symbol) at least 2 words.", "",
           "| case | GPU vs oracle, whole | GPU vs oracle, band | reference vs oracle, whole | reference vs oracle, band "
           "| max rel. diff GPU vs oracle | max rel. diff GPU vs reference |", "|---|---|---|---|---|---|---|"]
    stats = ["", "## Statistics of port 0", "", "| case | source | " + " | ".join(KEYS) + " |",
             "|---|---|" + "---|" * len(KEYS)]
    for case in cc.EDGE_CASES:
        grid, kw, est0, want, ws = cc.edge_args(case)
        cfg = amd.DmrsPuschEstimatorConfig(
            slot_index=kw["slot_index"], numerology=kw["numerology"], nof_tx_layers=kw["nof_layers"],
            scrambling_id=kw["scrambling_id"], n_scid=kw["n_scid"], scaling=kw["scaling"],
            symbols_mask=kw["symbols_mask"], rb_start=kw["prb_lo"], rb_count=kw["prb_hi"] - kw["prb_lo"],
            first_symbol=kw["first_symbol"], nof_symbols=kw["nof_symbols"], fd_smoothing=kw["fd"],
            td_interpolation=kw["td"], compensate_cfo=kw["compensate_cfo"])
        got, gs = est.estimate(grid, cfg, estimates=est0)
        band = cc.edge_band(kw, got.shape)
        rows = [("GPU", gs), ("oracle", ws)]
        if oracle.REF is not None:
            ref, rs = chest.ref_pusch_chest(grid, estimates=est0, **kw)
            rows.append(("reference", rs))
            rcols = [share(ref, want), share(ref, want, band)]
            gref = "%.2e" % max_rel(got, ref)
        else:
            rcols, gref = ["-", "-"], "-"
        out.append("| %s | %s | %s | %s | %s | %.2e | %s |" % (case[0], share(got, want), share(got, want, band),
                                                            rcols[0], rcols[1], max_rel(got, want), gref))
        for src, st in rows:
            stats.append("| %s | %s | " % (case[0], src) + " | ".join("%.7g" % float(st[0][k]) for k in KEYS) + " |")
    text = "\n".join(out + stats) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
