#!/usr/bin/env python3
"""Counterpart of the reference's ItemCF_Final.py on a synthetic ml-100k-shaped implicit split: k = 10 neighbours, top-20
lists for every user, recall / precision / F1 against the test split over users 0..n-2, divided by n, as ItemCF_Final.py:58 does.

    python scripts/itemcf.py
"""
import _common as c

from deeplearningrecommendationsystem_amd.cf import ItemCF, implicit_matrix, recall_precision_f1

train_u, train_i, test_u, test_i = c.implicit_split()
data = implicit_matrix(train_u, train_i, c.NUM_USERS, c.NUM_ITEMS, device=c.device)
model = ItemCF(k=10).fit(data)
recommendations = model.recommend(n=20)
recall, precision, f1 = recall_precision_f1(recommendations, test_u, test_i, users=range(c.NUM_USERS - 1), divisor=c.NUM_USERS)
print("recall, precision, F1:", recall, precision, f1)
