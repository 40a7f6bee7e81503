"""Borehole logs as a score of the kept models (gbp_borehole_score): what the kernel costs at a survey shape -- 256
attachments (one per attached sounding of 2048), n = 128 kept models of up to K = 64 layers, logs of 300 intervals between 0 and 150 m,
every other interval a lithology entry of 3 classes -- beside the numpy rule and beside a plain torch statement of the same rule.

The C entry is timed on preallocated buffers between device events (its host-side checks of the index arrays, which wait for the
stream, are inside the interval), medians after warm-up rounds.  The torch statement, in the same process, the two taking turns: the
overlap of every interval with every layer of every model as one clamped difference [attachments, intervals, models, layers], the class
posteriors per layer once per attachment, two reductions and a sum over the intervals, attachments in chunks that bound its memory;
its sums have another order, so it is compared within 1e-9 relative and the largest difference is written down.  The numpy rule
(``boreholes.score_reference``, fp64) is timed once on the first ``--rule-attachments`` attachments and scaled to all of them: it is a
statement of the rule, not an implementation anybody would run on a survey.  There is no pass / fail threshold: the kernel has no
parent; the numbers go into DESIGN.md 3.31.  Writes one JSON file.

    python scripts/bench_boreholes.py [--soundings 2048] [--attachments 256] [--models 128] [--layers 64] [--intervals 300] [--rounds 7]
                                      [--warmup 2] [--rule-attachments 4] [--seed 0] [--out profiles/boreholes/bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_spatial_sections import events_ms      # noqa: E402
from geobipy_amd import _lib, boreholes      # noqa: E402

CLASSES = (np.array([-2.0, -1.0, 0.0]), np.array([0.3, 0.3, 0.3]), np.array([1.0, 1.0, 1.0]))
FLOOR = 1e-6
TORCH_CHUNK = 8                                                                # attachments the torch statement takes at once


def problem(S, A, n, K, n_int, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(max(1, K // 4), K + 1, (S, n)).astype(np.int32)
    edges = np.sort(rng.uniform(0.5, 200.0, (S, n, K)), axis=2)
    sigma = 10.0 ** rng.uniform(-3.0, 0.5, (S, n, K))
    layer = np.arange(K)[None, None, :]
    edges = np.where(layer < k[:, :, None] - 1, edges, np.inf)
    sigma = np.where(layer < k[:, :, None], sigma, np.nan)
    rows, n_used = np.tile(np.arange(n, dtype=np.int32), (S, 1)), np.full(S, n, dtype=np.int32)
    cuts = np.sort(rng.uniform(0.0, 150.0, (A, n_int + 1)), axis=1)
    lith = (np.arange(n_int) % 2 == 1)[None, :].repeat(A, 0)
    logs = boreholes.Logs(rng.uniform(0, 1e4, A), rng.uniform(0, 1e4, A), None, np.arange(A + 1) * n_int, cuts[:, :-1].reshape(-1), cuts[:, 1:].reshape(-1),
                          np.where(lith, np.nan, rng.uniform(-3.0, 0.5, (A, n_int))).reshape(-1), np.where(lith, np.nan, 0.2).reshape(-1),
                          np.where(lith, rng.integers(0, 3, (A, n_int)), -1).reshape(-1))
    att_s = np.sort(rng.choice(S, A, replace=False))
    dist = rng.uniform(0.0, 150.0, A)
    att = dict(att_ptr=np.concatenate([[0], np.cumsum(np.bincount(att_s, minlength=S))]).astype(np.int32), att_sounding=att_s.astype(np.int32),
               att_bore=np.arange(A, dtype=np.int32), att_var=0.1 * 0.1 * dist / 100.0, att_shift=np.zeros(A), att_distance=dist)
    return k, edges, sigma, rows, n_used, att, logs


def torch_score(k, edges, sigma, att_s, var, top, bottom, value, sd, cls):
    """part [A, n] of the rule stated in torch (no shifts, every model present): tensors on the device, intervals [A, I]."""
    dev = k.device
    mu, sc, pr = (torch.as_tensor(a).to(dev) for a in CLASSES)
    A, n, K = att_s.numel(), k.shape[1], edges.shape[2]
    out = torch.empty((A, n), dtype=torch.float64, device=dev)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    for a0 in range(0, A, TORCH_CHUNK):
        sl = slice(a0, a0 + TORCH_CHUNK)
        s = att_s[sl]
        e, kk = edges[s], k[s]                                                 # [a, n, K]
        lay = torch.arange(K, device=dev)[None, None, :]
        bot = torch.where(lay < kk[:, :, None] - 1, e, inf)
        topl = torch.cat([torch.zeros_like(bot[:, :, :1]), bot[:, :, :-1]], dim=2)
        val = torch.where(lay < kk[:, :, None], torch.log10(sigma[s]), torch.zeros((), dtype=torch.float64, device=dev))
        t, b = top[sl][:, :, None, None], bottom[sl][:, :, None, None]        # [a, I, 1, 1]
        w = (torch.minimum(bot[:, None], b) - torch.maximum(topl[:, None], t)).clamp(min=0.0)      # [a, I, n, K]
        w = torch.where((lay < kk[:, :, None])[:, None], w, torch.zeros((), dtype=torch.float64, device=dev))
        h = (bottom[sl] - top[sl])[:, :, None]
        v = sc[None, :] ** 2 + var[sl][:, None]                                # [a, C]
        l = (torch.log(pr)[None, :] - 0.5 * torch.log(v))[:, :, None, None] - (val[:, None] - mu[None, :, None, None]) ** 2 / (2.0 * v)[:, :, None, None]
        P = torch.softmax(l, dim=1)                                            # [a, C, n, K]
        c = cls[sl].clamp(min=0)                                               # [a, I]
        Pc = torch.gather(P, 1, c[:, :, None, None].expand(-1, -1, n, K))      # [a, I, n, K]
        mean = (w * val[:, None]).sum(dim=3) / h
        pbar = (w * Pc).sum(dim=3) / h
        d = mean - torch.nan_to_num(value[sl])[:, :, None]
        meas = -(d * d) / (2.0 * (torch.nan_to_num(sd[sl], nan=1.0) ** 2 + var[sl][:, None]))[:, :, None]
        lith = torch.log(FLOOR + (1.0 - FLOOR) * pbar)
        out[sl] = torch.where((cls[sl] < 0)[:, :, None], meas, lith).sum(dim=1)
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--soundings", type=int, default=2048)
    p.add_argument("--attachments", type=int, default=256)
    p.add_argument("--models", type=int, default=128)
    p.add_argument("--layers", type=int, default=64)
    p.add_argument("--intervals", type=int, default=300)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rule-attachments", type=int, default=4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "boreholes", "bench.json"))
    a = p.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    S, A, n, K, I = a.soundings, a.attachments, a.models, a.layers, a.intervals
    k, edges, sigma, rows, n_used, att, logs = problem(S, A, n, K, I, a.seed)
    up = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)      # noqa: E731
    t = dict(k=up(k, np.int32), edges=up(edges, np.float64), sigma=up(sigma, np.float64), rows=up(rows, np.int32), nu=up(n_used, np.int32),
             aptr=up(att["att_ptr"], np.int32), abore=up(att["att_bore"], np.int32), avar=up(att["att_var"], np.float64), ashift=up(att["att_shift"], np.float64),
             bptr=up(logs.ptr, np.int32), top=up(logs.top, np.float64), bottom=up(logs.bottom, np.float64), value=up(logs.value, np.float64),
             sd=up(logs.sd, np.float64), cls=up(logs.cls, np.int32))
    score = torch.empty((S, n), dtype=torch.float64, device=dev)
    part = torch.empty((A, n), dtype=torch.float64, device=dev)
    skipped = torch.empty(A, dtype=torch.int32, device=dev)
    arr = lambda v: (ctypes.c_double * 16)(*v)                                 # noqa: E731
    c_mu, c_sc, c_ln = arr(CLASSES[0]), arr(CLASSES[1]), arr(np.log(CLASSES[2]))

    def kernel():
        _lib.call("gbp_borehole_score", dev, S, n, K, t["k"], t["edges"], t["sigma"], n, t["rows"], t["nu"], A, t["aptr"], t["abore"], t["avar"], t["ashift"], A,
                  t["bptr"], A * I, t["top"], t["bottom"], t["value"], t["sd"], t["cls"], 3, c_mu, c_sc, c_ln, FLOOR, score, part, skipped)

    att_s = up(att["att_sounding"], np.int64)
    shaped = {name: t[name].reshape(A, I) for name in ("top", "bottom", "value", "sd", "cls")}
    held = {}

    def statement():
        held["part"] = torch_score(t["k"], t["edges"], t["sigma"], att_s, t["avar"], shaped["top"], shaped["bottom"], shaped["value"], shaped["sd"], shaped["cls"])

    ms_kernel, ms_torch = [], []
    for r in range(a.warmup + a.rounds):
        mk, mt = events_ms(kernel, dev), events_ms(statement, dev)
        if r >= a.warmup:
            ms_kernel.append(mk), ms_torch.append(mt)
    diff = float(((part - held["part"]).abs() / part.abs().clamp(min=1.0)).max())
    assert diff <= 1e-9, diff
    assert int(skipped.abs().max()) == 0 and bool((score[att_s] == part).all())

    R = min(a.rule_attachments, A)
    sub = np.asarray(att["att_sounding"][:R])
    sub_att = dict(att_ptr=np.arange(R + 1, dtype=np.int32), att_sounding=np.arange(R, dtype=np.int32), att_bore=att["att_bore"][:R], att_var=att["att_var"][:R],
                   att_shift=att["att_shift"][:R], att_distance=att["att_distance"][:R])
    t0 = time.perf_counter()
    rule = boreholes.score_reference(k[sub], edges[sub], sigma[sub], rows[sub], n_used[sub], sub_att, logs, classes=CLASSES, class_floor=FLOOR)
    seconds_rule = (time.perf_counter() - t0) * A / R
    rule_diff = float(np.abs(rule["part"] - part[:R].cpu().numpy()).max())
    props = torch.cuda.get_device_properties(dev)
    out = dict(device=props.name, arch=getattr(props, "gcnArchName", ""), compute_units=props.multi_processor_count, soundings=S, attachments=A, models=n,
               layers=K, intervals_per_log=I, classes=3, rounds=a.rounds, warmup=a.warmup, waves=S * ((n + 63) // 64), working_waves=A * ((n + 63) // 64),
               lds_bytes_per_wave=64 * (2 * K - 1) * 8, ms_kernel=ms_kernel, ms_torch=ms_torch, seconds_kernel=float(np.median(ms_kernel)) / 1e3,
               seconds_torch=float(np.median(ms_torch)) / 1e3, seconds_numpy_rule_scaled=seconds_rule, numpy_rule_attachments_timed=R,
               torch_max_relative_difference=diff, numpy_rule_max_difference=rule_diff)
    out["torch_over_kernel"] = out["seconds_torch"] / out["seconds_kernel"]
    out["numpy_over_kernel"] = out["seconds_numpy_rule_scaled"] / out["seconds_kernel"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({name: v for name, v in out.items() if not name.startswith("ms_")}))
    return out


if __name__ == "__main__":
    main()
