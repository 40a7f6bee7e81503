"""Time of the horizon tracker (csrc/gbp_horizon.h k_horizon_viterbi, k_horizon_marginals) on a survey-sized launch -- 64 sequences of
1 024 soundings and 440 depth cells, planted dipping horizons under terrain with 30 % of the evidence at a wrong depth:

    python scripts/bench_horizons.py [--sequences 64 --soundings 1024 --states 440] [--reps 5] [--check 1]
                                     [--out profiles/horizons/bench.json]

  (a) gbp_horizon_track without marginals (the Viterbi kernel and its walk back), with marginals (both kernels), and with the absent
      state and marginals;
  (b) the torch formulation of the same steps on the device, batched over the sequences: per step a [L, S, S] gather of the 2 S - 1
      costs, then ``max`` over c (Viterbi, and N gathers for the walk back) or a batched ``matmul`` (forward and backward passes).

Every candidate runs on preallocated inputs, (a) through the C entry, and is timed with device events, the candidates alternating
inside each repetition of one process; medians after a warm-up.  The bar: (a) is faster than (b), the paths are equal, and the
marginals of (a) lie within the tolerance of tests/test_horizons_gpu.py of the long-double rule -- checked on ``--check`` sequences,
because the numpy rule takes about ten seconds per sequence of this size.  No counters are taken: with 64 workgroups on 256 CUs the
kernel is bound by the latency of its dependent steps by design.  Prints one line per measurement and writes them as JSON to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_intervals import alternating  # noqa: E402
from geobipy_amd import _lib, horizons  # noqa: E402


def planted(L, N, S, dz, seed):
    """Evidence [L N, S], x, surface [L N] of L lines with a dipping horizon each; 30 % of the soundings point at a random cell."""
    rng = np.random.default_rng(seed)
    x = np.tile(25.0 * np.arange(N), L)
    phase = np.repeat(rng.uniform(0.0, 6.0, L), N)
    surface = 10.0 * np.sin(x / 1500.0 + phase) + rng.normal(0.0, 0.3, L * N)
    depth = surface + 0.5 * S * dz - 10.0 - 6.0 * np.sin(x / 2000.0 + phase)
    true = np.clip(np.floor(depth / dz), 0, S - 1).astype(np.int64)
    at = np.where(rng.uniform(size=L * N) < 0.3, rng.integers(0, S, L * N), true)
    ev = 0.02 + np.exp(-0.5 * ((np.arange(S)[None, :] - at[:, None]) / 2.0) ** 2)
    return ev, x, surface, true


def torch_viterbi(score, g, d, dz, idx, kf):
    """score [L, N, S], g, d [L, N] -> (cell int64 [L, N], log_score [L]) by the rule's steps in torch."""
    L, N, S = score.shape
    V = score[:, 0]
    back = torch.empty((N, L, S), dtype=torch.int64, device=score.device)
    for n in range(N - 1):
        T = g[:, n, None] * torch.abs(d[:, n, None] - kf[None, :] * dz)                    # [L, 2 S - 1]
        m, arg = (V[:, None, :] - T[:, idx]).max(dim=2)                                    # [L, S', S] -> over c
        V = score[:, n + 1] + m
        back[n + 1] = arg
    top, cur = V.max(dim=1)
    cell = torch.empty((L, N), dtype=torch.int64, device=score.device)
    for n in range(N - 1, -1, -1):
        cell[:, n] = cur
        if n:
            cur = back[n].gather(1, cur[:, None])[:, 0]
    return cell, top


def torch_marginals(score, g, d, dz, idx, kf):
    """gamma [L, N, S] and log_partition [L] by the rule's scaled forward-backward in torch (batched matmul)."""
    L, N, S = score.shape
    w = torch.exp(score)
    alpha = torch.empty_like(score)
    s = torch.empty((L, N), dtype=torch.float64, device=score.device)
    a = w[:, 0]
    s[:, 0] = a.sum(dim=1)
    alpha[:, 0] = a / s[:, 0, None]
    for n in range(N - 1):
        K = torch.exp(-(g[:, n, None] * torch.abs(d[:, n, None] - kf[None, :] * dz)))[:, idx]      # [L, S', S]
        u = w[:, n + 1] * torch.bmm(K, alpha[:, n, :, None])[:, :, 0]
        s[:, n + 1] = u.sum(dim=1)
        alpha[:, n + 1] = u / s[:, n + 1, None]
    beta = torch.ones((L, S), dtype=torch.float64, device=score.device)
    gamma = torch.empty_like(score)
    for n in range(N - 1, -1, -1):
        if n < N - 1:
            K = torch.exp(-(g[:, n, None] * torch.abs(d[:, n, None] - kf[None, :] * dz)))[:, idx]
            beta = torch.bmm(K.transpose(1, 2), (w[:, n + 1] * beta)[:, :, None])[:, :, 0] / s[:, n + 1, None]
        gm = alpha[:, n] * beta
        gamma[:, n] = gm / gm.sum(dim=1, keepdim=True)
    return gamma, torch.log(s).sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--soundings", type=int, default=1024)
    ap.add_argument("--states", type=int, default=440)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=1, help="sequences whose marginals are held to the long-double numpy rule")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L, N, S, dz, slope, switch = a.sequences, a.soundings, a.states, 0.5, 0.05, 4.6
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ev, x, surface, true = planted(L, N, S, dz, 7)
    ptr = np.arange(L + 1, dtype=np.int64) * N
    score_h, _ = horizons.evidence_scores(ev)
    absent_h = np.full(L * N, np.log(0.01))
    g_h, d_h = horizons.steps(x, np.zeros(L * N), surface, slope, ptr=ptr)
    t = lambda v, dt=torch.float64: torch.as_tensor(v, dtype=dt).to(dev)                   # noqa: E731
    score, absent, g, d, tptr = t(score_h), t(absent_h), t(g_h), t(d_h), t(ptr, torch.int64)
    back = torch.empty((L * N, S + 1), dtype=torch.int16, device=dev)
    cell = torch.empty(L * N, dtype=torch.int32, device=dev)
    log_score = torch.empty(L, dtype=torch.float64, device=dev)
    marginal = torch.empty((L * N, S + 1), dtype=torch.float64, device=dev)
    log_partition = torch.empty(L, dtype=torch.float64, device=dev)
    scale = torch.empty(L * N, dtype=torch.float64, device=dev)

    def kernel(with_marginals, with_absent=False):
        p = (lambda v: v.data_ptr()) if with_marginals else (lambda v: None)
        _lib.check(lib.gbp_horizon_track(L, tptr.data_ptr(), L * N, N, S, dz, score.data_ptr(), absent.data_ptr() if with_absent else None,
                                         g.data_ptr(), d.data_ptr(), switch, back.data_ptr(), cell.data_ptr(), log_score.data_ptr(),
                                         p(marginal), p(log_partition), p(scale), stream))

    idx = (torch.arange(S, device=dev)[:, None] - torch.arange(S, device=dev)[None, :]) + (S - 1)       # [c', c] -> k + S - 1
    kf = torch.arange(-(S - 1), S, device=dev, dtype=torch.float64)
    s3, g2, d2 = score.view(L, N, S), g.view(L, N), d.view(L, N)
    keep = {}

    def tv():
        keep["viterbi"] = torch_viterbi(s3, g2, d2, dz, idx, kf)

    def tm():
        keep["marginals"] = torch_marginals(s3, g2, d2, dz, idx, kf)

    r = dict(sequences=L, soundings=N, states=S, reps=a.reps, device=torch.cuda.get_device_name(0))
    times = alternating({"kernel_viterbi": lambda: kernel(False), "kernel_both": lambda: kernel(True),
                         "kernel_both_absent": lambda: kernel(True, True), "torch_viterbi": tv, "torch_marginals": tm}, a.reps, warmup=2)
    for k, ms in times.items():
        r[k + "_ms"] = ms
    r["kernel_marginals_ms"] = times["kernel_both"] - times["kernel_viterbi"]
    r["kernel_viterbi_us_per_step"] = times["kernel_viterbi"] * 1e3 / (N - 1)
    r["kernel_marginals_us_per_step"] = r["kernel_marginals_ms"] * 1e3 / (N - 1)
    r["torch_viterbi_us_per_step"] = times["torch_viterbi"] * 1e3 / (N - 1)
    r["torch_marginals_us_per_step"] = times["torch_marginals"] * 1e3 / (N - 1)
    r["torch_over_kernel_viterbi"] = times["torch_viterbi"] / times["kernel_viterbi"]
    r["torch_over_kernel_marginals"] = times["torch_marginals"] / r["kernel_marginals_ms"]
    r["max_adds_per_launch"] = float(L) * (N - 1) * S * S
    # results: the paths equal, the marginals close to torch's and, on --check sequences, within the tests' bound of the rule
    kernel(True)
    torch.cuda.synchronize()
    tcell, ttop = keep["viterbi"]
    tgamma, tlp = keep["marginals"]
    r["path_equals_torch"] = bool(torch.equal(cell.view(L, N).long(), tcell))
    r["log_score_max_distance_to_torch"] = float((log_score - ttop).abs().max())
    err = np.abs(cell.view(L, N).cpu().numpy() - true.reshape(L, N))
    r["tracked_max_error_cells"], r["tracked_mean_error_cells"] = int(err.max()), float(err.mean())
    r["argmax_share_off_by_more_than_2"] = float(np.mean(np.abs(np.argmax(ev, axis=1) - true) > 2))
    # the kernel without the absent state against torch and the rule
    kernel(True, False)
    torch.cuda.synchronize()
    mk = marginal.view(-1)[: L * N * S].view(L, N, S)                      # (without absent_score the rows are S wide)
    r["marginal_max_distance_to_torch"] = float((mk - tgamma).abs().max())
    r["log_partition_max_distance_to_torch"] = float((log_partition - tlp).abs().max())
    e_max = dist_max = 0.0
    ok = True
    for l in range(min(a.check, L)):
        sl = slice(l * N, (l + 1) * N)
        ref = horizons.track_reference([0, N], score_h[sl], None, g_h[sl], d_h[sl], dz, switch)
        ld = horizons.track_reference([0, N], score_h[sl], None, g_h[sl], d_h[sl], dz, switch, dtype=np.longdouble)
        e = float(np.abs(ref["marginal"] - ld["marginal"]).max())
        dist = float(np.abs(mk[l].cpu().numpy() - ld["marginal"]).max())
        ok = ok and dist <= max(16.0 * e, 16.0 * 2.0 ** -52) and np.array_equal(cell.view(L, N)[l].cpu().numpy(), ref["cell"]) \
            and float(log_score[l]) == float(ref["log_score"][0])
        e_max, dist_max = max(e_max, e), max(dist_max, dist)
    r.update(checked_sequences=min(a.check, L), rule_own_rounding_e=e_max, marginal_max_distance_to_long_double_rule=dist_max,
             checked_sequences_meet_the_tolerance=bool(ok))
    r["kernel_meets_the_bar"] = bool(times["kernel_viterbi"] < times["torch_viterbi"] and r["kernel_marginals_ms"] < times["torch_marginals"]
                                     and r["path_equals_torch"] and ok)
    r["not_measured"] = "hardware counters, other launch sizes, more than one device"
    for k, v in r.items():
        print("%s: %s" % (k, ("%.4g" % v) if isinstance(v, float) else v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
