#!/usr/bin/env python3
"""Writes tests/golden/cf/usercf.npz and itemcf.npz from the reference's own UserCF_Final.py / ItemCF_Final.py.

Build container only (needs the reference tree and scikit-learn).  The scripts' top level reads Windows paths, so only
their ``def`` statements are taken (``ast``) and executed; no reference text is written anywhere.  Each fixture holds
the implicit split (packed bitmap + test pairs), k, n, the evaluated users and divisor, and two runs of the reference's
``recommendations_list`` / ``recommendations_list_item_based``:

  (a) with sklearn's ``cosine_similarity``, as the reference runs;
  (b) with this package's float32 similarity (tests/cf_numpy.py) upcast to float64 -- the reference's stable sort then
      sees the same ties, so its neighbours are ours and only the float64-vs-float32 prediction sums differ.

    python dev/make_cf_golden.py /path/to/reference
"""
import ast
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cf_numpy as cfn  # noqa: E402
from sklearn.metrics.pairwise import cosine_similarity  # noqa: E402

from deeplearningrecommendationsystem_amd import synth  # noqa: E402


def functions_of(path):
    tree = ast.parse(open(path, encoding="utf-8").read())
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
    ns = {}
    exec(compile(tree, path, "exec"), ns)
    return ns


def evaluate(recs, test_users, test_items, users, divisor):
    """the scripts' loop over users (recall over |test|, precision over |set(rec)|), sums divided by ``divisor``"""
    return np.array(cfn.metrics(recs, test_users, test_items, users, divisor))


def reference_neighbors(sim, k):
    out = []
    for row in sim:
        s = list(enumerate(row))
        s.sort(key=lambda x: x[1], reverse=True)
        out.append([x[0] for x in s[1:k + 1]])
    return np.array(out, dtype=np.int64)


def build(ref, kind, num_users, num_items, train_pairs, seed, users, divisor, out_name):
    k, n = 10, 20
    tu, ti, su, si = (t.numpy() for t in synth.implicit_split(num_users, num_items, train_pairs, 10, seed))
    data = cfn.dense(tu, ti, num_users, num_items).astype(np.int64)
    assert data.any(1).all() and data.any(0).all(), "every user and item must occur in training"
    if kind == "user":
        fn = functions_of(os.path.join(ref, "UserCF_Final.py"))["recommendations_list"]
        rows = data
    else:
        fn = functions_of(os.path.join(ref, "ItemCF_Final.py"))["recommendations_list_item_based"]
        rows = data.T
    sim_a = cosine_similarity(rows)
    sim_b = cfn.similarity(rows.astype(np.uint8)).astype(np.float64)
    res = {}
    for tag, sim in (("a", sim_a), ("b", sim_b)):
        t = time.time()
        recs, preds = [], []
        for u in users:
            r = fn(data, sim, int(u), k, n)
            recs.append([x[0] for x in r] + [-1] * (n - len(r)))
            preds.append([x[1] for x in r] + [0.0] * (n - len(r)))
        full = np.full((num_users, n), -1, dtype=np.int64)
        full[users] = recs
        res[tag] = (np.array(recs, dtype=np.int16), np.array(preds, dtype=np.float32),
                    evaluate(full, su, si, users, divisor), reference_neighbors(sim, k))
        print(f"{out_name} ({tag}): {time.time() - t:.1f} s, metrics {res[tag][2]}")
    sample = np.arange(0, rows.shape[0], max(1, rows.shape[0] // 8))[:8]
    bitmap = np.packbits(data.astype(np.uint8).reshape(-1))
    meta = dict(kind=kind, source=f"{'UserCF' if kind == 'user' else 'ItemCF'}_Final.py", seed=seed)
    path = os.path.join(ROOT, "tests", "golden", "cf", out_name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(
        path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), bitmap=bitmap,
        num_users=num_users, num_items=num_items, k=k, n=n, users=np.asarray(users, dtype=np.int64),
        divisor=divisor, test_users=su.astype(np.int16), test_items=si.astype(np.int16),
        a_recs=res["a"][0], a_metrics=res["a"][2], a_neighbors=res["a"][3].astype(np.int16),
        b_recs=res["b"][0], b_preds=res["b"][1], b_metrics=res["b"][2], b_neighbors=res["b"][3].astype(np.int16),
        sim_rows=sample, sim_sample=sim_a[sample])
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CF_REFERENCE_DIR", "")
    build(ref, "user", 943, 1682, 90_570, 5, np.arange(943), 943, "usercf.npz")
    # ItemCF_Final.py:58 evaluates users 1..n-1 (0-based 0..n-2) and divides by n
    build(ref, "item", 200, 400, 8_000, 6, np.arange(199), 200, "itemcf.npz")
