"""Torch formulation of what csrc/gbp_hitmap.h's k_hitmap_classes computes (test infrastructure: the kernel is held to it on shapes the
reference fixture does not cover, and it to the imported reference's own class probabilities, tests/golden/class_probability.npz;
tests/test_class_probability.py)."""
import math

import numpy as np
import torch


def class_probability_torch(hitmap, log_mean_prior, half_width, means, scales):
    """probability [B, K, nz], highest_marginal [B, nz] (int32) and probability_of_highest_marginal [B, nz] of the hit maps
    [B, n_value, n_depth]: x_v = ((v + 0.5) / nv) 2 hw - hw + log_mean_prior / ln 10, phi_k = scipy's norm.pdf(x_v, means[k], scales[k]),
    S_k = sum_v c_v phi_k(x_v), P_k = S_k / sum_k S_k (0 / 0 = NaN); the argmax over the class axis with numpy's rules."""
    B, nv, nz = hitmap.shape
    dev = hitmap.device
    mu = torch.as_tensor(np.asarray(means, dtype=np.float64), device=dev)
    sd = torch.as_tensor(np.asarray(scales, dtype=np.float64), device=dev)
    K = mu.numel()
    shift = torch.as_tensor(np.asarray(log_mean_prior.cpu(), dtype=np.float64) / 2.302585092994046, device=dev)
    c = (torch.arange(nv, dtype=torch.float64, device=dev) + 0.5) / nv * (2.0 * half_width) - half_width
    x = c[None, :] + shift[:, None]                                               # [B, nv]
    y = (x[:, None, :] - mu[None, :, None]) / sd[None, :, None]                   # [B, K, nv]
    phi = torch.exp(-y * y / 2.0) / math.sqrt(2.0 * math.pi) / sd[None, :, None]
    S = torch.bmm(phi, hitmap.to(torch.float64))                                  # [B, K, nz]
    P = S / S.sum(dim=1, keepdim=True)
    if B == 0:
        return dict(probability=P, highest_marginal=torch.zeros((0, nz), dtype=torch.int32, device=dev),
                    probability_of_highest_marginal=torch.zeros((0, nz), dtype=torch.float64, device=dev))
    j = torch.as_tensor(np.argmax(P.cpu().numpy(), axis=1).astype(np.int32), device=dev)   # numpy's: first max, a NaN wins
    best_p = torch.gather(P, 1, j[:, None].long())[:, 0]
    assert K >= 1
    return dict(probability=P, highest_marginal=j, probability_of_highest_marginal=best_p)
