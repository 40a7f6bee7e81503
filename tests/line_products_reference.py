"""Torch formulation of what csrc/gbp_hitmap.h's k_hitmap_products computes (test infrastructure: the kernel is held to it on shapes the
reference fixture does not cover, and it -- with the finishing functions of geobipy_amd/line_products.py -- to the imported reference's own
numbers, tests/golden/line_products.npz; tests/test_line_products.py)."""
import numpy as np
import torch


def moments_torch(hitmap, log_mean_prior, half_width, q):
    """mean, mode_idx, q_idx [len(q), B, nz], total (int64), s1 = sum c ln c of the hit maps [B, n_value, n_depth] along the value axis."""
    B, nv, nz = hitmap.shape
    centres = (torch.arange(nv, dtype=torch.float64, device=hitmap.device) + 0.5) / nv * (2.0 * half_width) - half_width
    h = hitmap.transpose(1, 2).to(torch.float64)                  # [B, nz, nv]
    total = hitmap.to(torch.int64).sum(dim=1)
    t = total.to(torch.float64).clamp(min=1.0)
    mean = (h * centres).sum(dim=2) / t + (log_mean_prior / np.log(10.0))[:, None]
    mode_idx = torch.argmax(hitmap.transpose(1, 2), dim=2).to(torch.int32)     # first of the maxima, as numpy
    cdf = torch.cumsum(hitmap.transpose(1, 2).to(torch.int64), dim=2).to(torch.float64) / t[:, :, None]
    q_idx = torch.stack([(cdf < qk).sum(dim=2).clamp(max=nv - 1) for qk in q]).to(torch.int32) if len(q) else \
        torch.empty((0, B, nz), dtype=torch.int32, device=hitmap.device)
    s1 = torch.where(h > 0, h * torch.log(torch.where(h > 0, h, torch.ones_like(h))), torch.zeros_like(h)).sum(dim=2)
    return dict(mean=mean, mode_idx=mode_idx, q_idx=q_idx, total=total, s1=s1)
