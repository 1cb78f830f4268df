#!/usr/bin/env python3
"""Counterpart of the reference's GDCF_Final.py on a synthetic ml-100k-shaped implicit split: k = 100, lr = 0.01,
10 epochs of Adam on the BCEWithLogits loss over the whole user x item matrix; per epoch the loss and the recall,
precision and F1 of the top 50 items of the scores formed before that epoch's step (training items not excluded),
divided by the number of users (GDCF_Final.py:48-95).  No plotting.

    python scripts/gdcf.py
"""
import _common as c

from deeplearningrecommendationsystem_amd import GDCF, implicit_matrix, optim, recall_precision_f1

embedding_size, lr, n = 100, 0.01, 10
train_u, train_i, test_u, test_i = c.implicit_split()
data = implicit_matrix(train_u, train_i, c.NUM_USERS, c.NUM_ITEMS, device=c.device)
model = GDCF(c.NUM_USERS, c.NUM_ITEMS, embedding_size, seed=0, device=c.device)
optimizer = optim.Adam(model.parameters(), lr=lr)
for n_iter in range(n):
    loss = model(data)
    loss.backward()
    top = model.recommend(n=50)          # P and Q as they were before this epoch's step
    optimizer.step()
    optimizer.zero_grad()
    recall, precision, f1 = recall_precision_f1(top, test_u, test_i)
    print(f"epoch {n_iter + 1} loss {loss.item():.6f} recall {recall:.6f} precision {precision:.6f} F1 {f1:.6f}")
