"""bench.py --dump-outputs DIR: what the timed path computed in its last timed step, as DIR/<name>.npy."""
import os

import numpy as np

DUMP_BUDGET_BYTES = 60 << 20    # all of a run's files together stay below 64 MB


def dump_outputs(args, rank, outputs):
    """Writes the arrays the timed path handed back in its last timed step, DIR/<name>.npy each (rank 0's batch).
    `outputs` (a dict, or a callable that returns it and is called only when files are wanted) maps a name to a
    torch tensor or numpy array as the caller of the path holds it: complex values are stored as (re, im) pairs,
    floats and integers up to 16 bits as float32, wider integers as float64.  The byte budget is split evenly over
    the arrays; one that exceeds its share is stored as a fixed sample: the elements at the sorted flat indices drawn
    by numpy's default_rng(0), the same for every run of a given shape.  The benchmark's inputs are seeded, so two
    builds run with the same arguments can be compared file by file."""
    out_dir = getattr(args, "dump_outputs", None)
    if not out_dir or rank != 0:
        return
    import torch

    if callable(outputs):
        outputs = outputs()

    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BUDGET_BYTES // len(outputs)
    for name, a in outputs.items():
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.is_complex():
            t = torch.view_as_real(t)
        wide = t.dtype in (torch.int32, torch.int64, torch.float64)
        flat = t.reshape(-1)
        cap = share // (8 if wide else 4)
        if flat.numel() > cap:
            idx = np.sort(np.random.default_rng(0).integers(0, flat.numel(), cap))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        else:
            flat = flat.reshape(t.shape)
        np.save(os.path.join(out_dir, name + ".npy"),
                flat.to(torch.float64 if wide else torch.float32).cpu().numpy())


def records_to_columns(raw, dtype):
    """uint8 [n][record] result records (torch or numpy) -> float64 [n][fields], nested records flattened in order."""
    if hasattr(raw, "cpu"):
        raw = raw.cpu().numpy()
    rec = np.ascontiguousarray(raw).view(np.dtype(dtype)).reshape(-1)

    def cols(r):
        out = []
        for n in r.dtype.names:
            out += cols(r[n]) if r[n].dtype.names else [r[n].astype(np.float64).reshape(r.shape[0], -1)]
        return out

    return np.concatenate(cols(rec), axis=1)
