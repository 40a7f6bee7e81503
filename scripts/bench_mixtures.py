"""Time of the local mixture fits (csrc/gbp_hitmap.h k_hitmap_mixture) on the synthetic layered hit maps of
bench_line_products.py -- 8 192 maps of 250 x 440 and a block of 1 024 --, Kmax = 3 and 50 iterations, against (a) the torch
formulation of the same rule on the device (``mixture_torch``: every cell of every column, chunked over the soundings) and (b)
k_hitmap_classes at K = 1 on the same maps, the scale of one read of them:

    python scripts/bench_mixtures.py [--B 8192] [--block 1024] [--reps 10] [--torch-soundings 256] [--out profiles/mixtures/bench.json]

The kernels are launched through their C entries on preallocated buffers and timed with device events, one launch per event pair, the
candidates alternating inside each repetition of one process; the figures are medians after a warm-up.  The torch formulation is timed
on the first --torch-soundings maps of the block and scaled by the sounding count (its cost per sounding does not depend on the block).
The condition: the kernel is faster than the torch formulation.  Flops are counted from the rule, an add, multiply, divide or compare
as 1 and an exp or log as 25: per non-empty cell, component and iteration 63 (+ 28 per cell), per cell and component of the closing
pass 31 (+ 65 per cell).  Prints one line per measurement and writes them as JSON to --out."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_intervals import alternating  # noqa: E402
from bench_line_products import layered_maps  # noqa: E402
from geobipy_amd import _lib, line_products, mixtures  # noqa: E402

FP64_VECTOR_TFLOPS = 78.6                       # MI355X, the data sheet's figure
TINY = 10.0 * 2.0 ** -52


def stage_torch(c, x, N, K, n_iter, reg, dx):
    """Stage K of the rule in torch for counts c [nv, C] (float64) on their device: (weight, mean, variance [K, C], loglik, ll_change
    [C], misfit [2, C]) -- geobipy_amd/mixtures.py _stage, operation for operation, over every cell."""
    nv, C = c.shape
    pos = c > 0
    m = (c * x[:, None]).sum(dim=0) / N
    dm = x[:, None] - m[None, :]
    V = (c * dm * dm).sum(dim=0) / N

    def e_step(w, mu, s2):
        d = x[None, :, None] - mu[:, None, :]
        ell = (torch.log(w) - 0.5 * torch.log(2.0 * np.pi * s2))[:, None, :] - d * d / (2.0 * s2)[:, None, :]
        return d, ell, torch.logsumexp(ell, dim=0)

    if K == 1:
        w, mu, s2, ll_prev = torch.ones((1, C), dtype=c.dtype, device=c.device), m[None, :], (V + reg)[None, :], None
    else:
        cum = torch.cumsum(c.to(torch.int64), dim=0)
        Ni = N.to(torch.int64)
        idx = torch.stack([(2 * K * cum < (2 * j + 1) * Ni[None, :]).sum(dim=0) for j in range(K)]).clamp(max=nv - 1)
        w = torch.full((K, C), 1.0 / K, dtype=c.dtype, device=c.device)
        mu = x[idx]
        s2 = (V / float(K * K) + reg)[None, :].repeat(K, 1)
        for _ in range(n_iter):
            d, ell, L = e_step(w, mu, s2)
            r = torch.where(pos[None], c[None] * torch.exp(ell - L[None]), torch.zeros((), dtype=c.dtype, device=c.device))
            ll_prev = torch.where(pos, c * L, torch.zeros((), dtype=c.dtype, device=c.device)).sum(dim=0) / N
            n = r.sum(dim=1) + TINY
            g = (r * d).sum(dim=1) / n
            mu = mu + g
            s2 = ((r * d * d).sum(dim=1) / n - g * g).clamp(min=0.0) + reg
            w = n / n.sum(dim=0, keepdim=True)
    L = e_step(w, mu, s2)[2]
    loglik = (c * L).sum(dim=0) / N
    p = c / N[None, :]
    e = (p - torch.exp(L) * dx).abs()
    misfit = torch.stack([e.max(dim=0).values / p.max(dim=0).values, (e * e).sum(dim=0).sqrt() / (p * p).sum(dim=0).sqrt()])
    change = torch.zeros_like(loglik) if ll_prev is None else loglik - ll_prev
    nan = torch.full((), float("nan"), dtype=c.dtype, device=c.device)
    return tuple(torch.where(N == 0, nan, v) for v in (w, mu, s2, loglik, change, misfit))


def mixture_torch(hm, half_width, Kmax, n_iter, chunk=32):
    """The stages of ``hitmap.mixture`` by torch operations on the maps' device, ``chunk`` soundings at a time."""
    B, nv, nz = hm.shape
    x = torch.as_tensor(mixtures.centres(nv, half_width), device=hm.device)
    dx = 2.0 * half_width / nv
    reg = dx * dx / 12.0
    S = Kmax * (Kmax + 1) // 2
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=hm.device)      # noqa: E731
    out = dict(weight=f64(B, S, nz), mean=f64(B, S, nz), sd=f64(B, S, nz), loglik=f64(B, Kmax, nz), ll_change=f64(B, Kmax, nz),
               misfit=f64(B, Kmax, 2, nz))
    for b0 in range(0, B, chunk):
        h = hm[b0:b0 + chunk]
        n = h.shape[0]
        c = h.permute(1, 0, 2).reshape(nv, n * nz).to(torch.float64)
        N = c.sum(dim=0)
        for K in range(1, Kmax + 1):
            w, mu, s2, ll, ch, mf = stage_torch(c, x, N, K, n_iter, reg, dx)
            s0 = K * (K - 1) // 2
            out["weight"][b0:b0 + n, s0:s0 + K] = w.view(K, n, nz).permute(1, 0, 2)
            out["mean"][b0:b0 + n, s0:s0 + K] = mu.view(K, n, nz).permute(1, 0, 2)
            out["sd"][b0:b0 + n, s0:s0 + K] = s2.sqrt().view(K, n, nz).permute(1, 0, 2)
            out["loglik"][b0:b0 + n, K - 1] = ll.view(n, nz)
            out["ll_change"][b0:b0 + n, K - 1] = ch.view(n, nz)
            out["misfit"][b0:b0 + n, K - 1] = mf.view(2, n, nz).permute(1, 0, 2)
    return out


def counted_flops(hm, Kmax, n_iter):
    """Flops of the rule on these maps under the convention of the module's header."""
    nnz, cells = int((hm > 0).sum()), hm.numel()
    em = sum(nnz * n_iter * (63 * K + 28) for K in range(2, Kmax + 1))
    closing = sum(cells * (31 * K + 65) for K in range(1, Kmax + 1))
    return em + closing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-soundings", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nv, nz, hw, Kmax, n_iter = 250, 440, 2.3, 3, 50
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    dx = 2.0 * hw / nv
    reg = dx * dx / 12.0
    S = Kmax * (Kmax + 1) // 2
    r = dict(n_value=nv, n_depth=nz, max_components=Kmax, n_iter=n_iter, reps=a.reps, device=torch.cuda.get_device_name(0))
    mu_, sd_ = (ctypes.c_double * 1)(-2.0), (ctypes.c_double * 1)(0.4)
    for tag, B in (("line", a.B), ("block", a.block)):
        hm = layered_maps(B, nv, nz, dev)
        lmp = torch.full((B,), -2.0 * line_products.LN10, dtype=torch.float64, device=dev)
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
        out = dict(weight=f64(B, S, nz), mean=f64(B, S, nz), sd=f64(B, S, nz), loglik=f64(B, Kmax, nz), ll_change=f64(B, Kmax, nz),
                   misfit=f64(B, Kmax, 2, nz))
        prob, best, best_p = f64(B, 1, nz), torch.empty((B, nz), dtype=torch.int32, device=dev), f64(B, nz)

        def mixture():
            _lib.check(lib.gbp_hitmap_mixture(B, nv, nz, hm.data_ptr(), hw, Kmax, n_iter, reg, out["weight"].data_ptr(), out["mean"].data_ptr(),
                                              out["sd"].data_ptr(), out["loglik"].data_ptr(), out["ll_change"].data_ptr(),
                                              out["misfit"].data_ptr(), stream))

        def classes_1():
            _lib.check(lib.gbp_hitmap_classes(B, nv, nz, hm.data_ptr(), lmp.data_ptr(), hw, 1, mu_, sd_, prob.data_ptr(), best.data_ptr(),
                                              best_p.data_ptr(), stream))

        t = alternating({"mixture": mixture, "classes_1": classes_1}, a.reps, warmup=2)
        nt = min(B, a.torch_soundings)
        tt = alternating({"torch": lambda: mixture_torch(hm[:nt], hw, Kmax, n_iter)}, 2, warmup=1)["torch"]
        flops = counted_flops(hm, Kmax, n_iter)
        p = tag + "_"
        r[p + "soundings"], r[p + "columns"] = B, B * nz
        r[p + "median_non_empty_cells"] = float((hm > 0).sum(dim=1).to(torch.float64).median())
        r[p + "mixture_ms"], r[p + "classes_1_ms"] = t["mixture"], t["classes_1"]
        r[p + "torch_soundings_timed"], r[p + "torch_ms_timed"] = nt, tt
        r[p + "torch_ms_scaled"] = tt * B / nt
        r[p + "column_iterations_per_s"] = B * nz * n_iter / (t["mixture"] * 1e-3)
        r[p + "torch_over_mixture"] = r[p + "torch_ms_scaled"] / t["mixture"]
        r[p + "mixture_over_classes_1"] = t["mixture"] / t["classes_1"]
        r[p + "counted_flops"] = flops
        r[p + "fraction_of_fp64_vector_peak"] = flops / (t["mixture"] * 1e-3) / (FP64_VECTOR_TFLOPS * 1e12)
        r[p + "mixture_faster_than_torch"] = bool(t["mixture"] < r[p + "torch_ms_scaled"])
        if tag == "block":                        # a check of what was timed: the kernel against torch and against the host rule on a slice
            ref_t = mixture_torch(hm[:8], hw, Kmax, n_iter)
            ref_h = mixtures.mixture_reference(hm[:8].cpu().numpy(), hw, Kmax, n_iter)
            for k in ("weight", "mean", "sd"):
                r["check_%s_against_torch" % k] = float(torch.nan_to_num(out[k][:8] - ref_t[k]).abs().max())
                r["check_%s_against_host_rule" % k] = float(np.nanmax(np.abs(out[k][:8].cpu().numpy() - ref_h[k])))
        del hm, out, prob, best, best_p
        torch.cuda.empty_cache()
    for k_, v in r.items():
        print("%s: %s" % (k_, ("%.4g" % v) if isinstance(v, float) else v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
