#!/usr/bin/env python3
"""Writes tests/golden/gdcf/gdcf_ml100k.npz from a run of the reference's own GDCF_Final.py.

Build container only (needs the reference tree, pandas and matplotlib).  The script is executed as it stands on a
synthetic ml-100k-shaped split: ``pd.read_csv`` is patched to return the split (1-based ids, as the files hold them),
matplotlib draws to the Agg backend and ``plt.show`` does nothing, stdout is silenced, and numpy's legacy global RNG
is seeded first, so P0 = rand(m, k) and Q0 = rand(n, k) can be redrawn from the seed.  No reference text is written
anywhere.  The fixture holds the packed train bitmap, the test pairs, the seed and hyper-parameters, the per-epoch
losses / recalls / precisions / F1s, sampled rows of the final P and Q and float64 checksums of both.

    python dev/make_gdcf_golden.py /path/to/reference/GDCF_Final.py
"""
import contextlib
import io
import json
import os
import runpy
import sys
import time

import matplotlib
import numpy as np

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import pandas as pd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deeplearningrecommendationsystem_amd import synth  # noqa: E402


def build(script, num_users, num_items, train_pairs, split_seed, seed, out_name):
    tu, ti, su, si = (t.numpy() for t in synth.implicit_split(num_users, num_items, train_pairs, 10, split_seed))
    base = pd.DataFrame({"userId": tu + 1, "itemId": ti + 1, "rating": np.full(tu.shape, 4, dtype=np.int64),
                         "timestamp": np.zeros(tu.shape, dtype=np.int64)})
    test = pd.DataFrame({"user_id": su + 1, "item_id": si + 1})

    def read_csv(path, *args, **kwargs):
        return (test if kwargs.get("usecols") is not None else base).copy()

    real_read_csv, real_show = pd.read_csv, plt.show
    pd.read_csv, plt.show = read_csv, (lambda *a, **k: None)
    try:
        np.random.seed(seed)
        t = time.time()
        with contextlib.redirect_stdout(io.StringIO()):
            g = runpy.run_path(script, run_name="__main__")
    finally:
        pd.read_csv, plt.show = real_read_csv, real_show
    P = g["P"].detach().numpy()
    Q = g["Q"].detach().numpy().T.copy()   # the script keeps Q.T
    k = P.shape[1]
    assert P.shape == (num_users, k) and Q.shape == (num_items, k)
    rows_p = np.unique(np.r_[np.linspace(0, num_users - 1, 12).astype(np.int64), num_users - 1])
    rows_q = np.unique(np.r_[np.linspace(0, num_items - 1, 12).astype(np.int64), num_items - 1])
    data = np.zeros((num_users, num_items), dtype=np.uint8)
    data[tu, ti] = 1
    meta = dict(source="GDCF_Final.py", split_seed=split_seed)
    path = os.path.join(ROOT, "tests", "golden", "gdcf", out_name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(
        path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
        bitmap=np.packbits(data.reshape(-1)), num_users=num_users, num_items=num_items, seed=seed, k=k,
        lr=float(g["lr"]), epochs=int(g["n"]), test_users=su.astype(np.int16), test_items=si.astype(np.int16),
        losses=np.array(g["losses"]), recalls=np.array(g["Recalls"]), precisions=np.array(g["Precisions"]),
        f1s=np.array(g["F1s"]), rows_p=rows_p, p_rows=P[rows_p], rows_q=rows_q, q_rows=Q[rows_q],
        p_sum=P.sum(), q_sum=Q.sum(), p_abs_sum=np.abs(P).sum(), q_abs_sum=np.abs(Q).sum())
    print(f"{path}: {os.path.getsize(path)} bytes, {time.time() - t:.1f} s, losses {g['losses'][0]:.6f} .. "
          f"{g['losses'][-1]:.6f}, recall {g['Recalls'][-1]:.6f}")


if __name__ == "__main__":
    script = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GDCF_REFERENCE_SCRIPT", "")
    build(script, 943, 1682, 90_570, 5, 2024, "gdcf_ml100k.npz")
