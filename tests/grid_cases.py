"""Inputs, references and error measures that the grid-scorer GPU tests share: tests/test_gpu_grid_scorer.py and
tests/test_gpu_{ncf,din,dien,deepfm,pnn}_grid.py.  A plain module, not a conftest: it defines no fixture and no test."""
import numpy as np
import torch

DEV = "cuda:0"
RTOL, ATOL = 1e-5, 1e-6      # the project's tolerance for prob (tests/test_gpu_models.py)


def observed(nu, ni, seed=3):
    """an ObservedPairs with user 0 having seen everything, user 1 all but two items, the others a random third"""
    from deeplearningrecommendationsystem_amd.data import ObservedPairs
    seen = torch.rand((nu, ni), generator=torch.Generator().manual_seed(seed)) < 0.33
    seen[0] = True
    seen[1] = True
    seen[1, [2, ni - 1]] = False
    u, i = seen.nonzero(as_tuple=True)
    return ObservedPairs(u.to(DEV), i.to(DEV), nu, ni), seen.numpy()


def features(nu, ni, gen):
    """(user_features (nu, 24), item_features (ni, 19)) float32: age uniform, gender and occupation one-hot, genres
    Bernoulli(0.09), item 1 without a genre"""
    uf = torch.zeros((nu, 24))
    uf[:, 0] = torch.rand(nu, generator=gen)
    uf[torch.arange(nu), 1 + torch.randint(0, 2, (nu,), generator=gen)] = 1.0
    uf[torch.arange(nu), 3 + torch.randint(0, 21, (nu,), generator=gen)] = 1.0
    itf = (torch.rand((ni, 19), generator=gen) < 0.09).float()
    if ni > 1:
        itf[1] = 0.0
    return uf, itf


def frame(uf, itf):
    """the full (nu * ni, 45) feature frame, user-major"""
    nu, ni = uf.shape[0], itf.shape[0]
    u = torch.arange(nu).repeat_interleave(ni)
    i = torch.arange(ni).repeat(nu)
    return torch.cat([u[:, None].to(uf.dtype), i[:, None].to(uf.dtype), uf[u], itf[i]], dim=1)


def histories(rows, ni, length, seed):
    hist = torch.randint(0, ni, (rows, length), generator=torch.Generator().manual_seed(seed))
    if rows >= 2:
        hist[0] = hist[0, 0]                      # one repeated id
        hist[-1, length // 2] = 0                 # id 0 is a real row
    return hist


def forward_pairs(model, hist, ni):
    with torch.no_grad():
        return model(hist.repeat_interleave(ni, 0), torch.arange(ni, device=DEV).repeat(hist.shape[0])).view(-1, ni)


def rank64(scores64, allowed=None):
    """float64 ranking, best first, ties by ascending id; rows of ``allowed`` False rank last"""
    s = np.where(allowed, scores64, -np.inf) if allowed is not None else scores64
    return np.argsort(-s, axis=1, kind="stable")


def frac_of_bound(got, want, atol):
    """worst |error| / (atol + rtol |want|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (atol + RTOL * np.abs(want))).max()) if want.size else 0.0


def error_and_frac(got, scores64):
    """(worst |error|, worst |error| / (atol + rtol |scores64|)) of a device tensor of scores"""
    err = np.abs(got.cpu().numpy().astype(np.float64) - scores64)
    return err.max(), (err / (ATOL + RTOL * np.abs(scores64))).max()
