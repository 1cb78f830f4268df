#!/usr/bin/env python3
"""Writes tests/golden/group_eval/small.npz from the reference's own evaluator/ranking.py (Ranking).

Build container only (needs the reference tree).  Only the ``Ranking`` class is taken (``ast``) and executed; no
reference text is written anywhere.

  small.npz   two score sets of N = 200 groups of 1 + k = 10 candidates (slot 0 the positive): integer-valued scores
              from {0..5}, so most groups have ties, and the same with +inf / -inf put at positives and negatives.
              Per set: the scores, the pessimistic ordering of every group's candidate slots (the negatives that are
              not below the positive in slot order, then the positive, then the rest), and the reference's numbers
              for ``Ranking([[0]] * N, orderings, c)``, c in {1, 3, 10, 20}: Recall@c, Mean NDCG@c, MAP@c, and MRR.
              With one relevant item per group these are HR@c, NDCG@c, MRR@c and MRR of the sampled protocol.

    python dev/make_group_eval_golden.py /path/to/reference
"""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFFS = (1, 3, 10, 20)


def reference(ref):
    ns = {"np": np}
    path = os.path.join(ref, "evaluator", "ranking.py")
    tree = ast.parse(open(path, encoding="utf-8").read())
    tree.body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Ranking"]
    exec(compile(tree, path, "exec"), ns)
    return ns["Ranking"]


def pessimistic_order(row):
    """candidate slots of one group, best first, every tie against the positive (slot 0)"""
    pos = row[0]
    ahead = [j for j in range(1, len(row)) if not row[j] < pos]
    behind = [j for j in range(1, len(row)) if row[j] < pos]
    return ahead + [0] + behind


def evaluate(Ranking, scores, tag, out):
    order = np.array([pessimistic_order(r) for r in scores], dtype=np.int16)
    real = [[0]] * len(scores)
    rec = [[int(x) for x in r] for r in order]
    out[f"{tag}_scores"] = scores
    out[f"{tag}_order"] = order
    rows = []
    for c in CUTOFFS:
        r = Ranking(real, rec, c)
        rows.append([r.precision_recall_f1()[1], r.mean_ndcg(), r.mapk()])
    out[f"{tag}_recall_ndcg_map"] = np.array(rows, dtype=np.float64)
    out[f"{tag}_mrr"] = np.float64(Ranking(real, rec, CUTOFFS[0]).mrr())


def build(Ranking):
    n, k = 200, 9
    gen = np.random.default_rng(37)
    ties = gen.integers(0, 6, (n, 1 + k)).astype(np.float32)
    ties[0] = 3.0                     # all equal: rank k
    ties[1] = 2.0
    ties[1, 0] = 5.0                  # strictly best positive: rank 0
    inf = ties.copy()
    inf[gen.integers(0, n, 30), 0] = np.inf
    inf[gen.integers(0, n, 30), 0] = -np.inf
    inf[gen.integers(0, n, 60), gen.integers(1, 1 + k, 60)] = np.inf
    inf[gen.integers(0, n, 60), gen.integers(1, 1 + k, 60)] = -np.inf
    out = dict(cutoffs=np.array(CUTOFFS, dtype=np.int64), negatives=np.int64(k))
    evaluate(Ranking, ties, "ties", out)
    evaluate(Ranking, inf, "inf", out)
    return out


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RANKING_REFERENCE_DIR", "")
    out = build(reference(ref))
    os.makedirs(os.path.join(ROOT, "tests", "golden", "group_eval"), exist_ok=True)
    meta = dict(source="evaluator/ranking.py", case="small")
    path = os.path.join(ROOT, "tests", "golden", "group_eval", "small.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **out)
    print(path, os.path.getsize(path), "bytes")
