"""Connected bodies of joint realisations (gbp_bodies_label): what labelling costs on the survey of
bench_spatial_draws.py (40 lines x 250 soundings, R = 64 realisations) at 55 and 440 columns, with the along-line edges (40 groups: one
workgroup per line and realisation) and with the whole survey graph (one group: one workgroup per realisation).

The C entry is timed on preallocated buffers between device events, medians after warm-up rounds.  The yardstick is the torch
statement of the same rule, in the same process, the two taking turns: the cell pairs with both cells members (vertical and across
every edge), min-propagation over them by ``scatter_reduce_(amin)`` in both directions plus one step of pointer jumping per round,
iterated until a round changes nothing (one host synchronisation per round), realisations in chunks that bound its memory.  Its labels
must be ``torch.equal`` to the kernel's.  The realisations are independent picks of every sounding's models (the ensemble of
bench_spatial_sections.py, where 30 % of the soundings carry a decoy family 15 m off): bodies with steps and gaps, not joint draws --
the cost of labelling depends on the raster, not on how it was drawn.  There is no pass / fail threshold: the kernel has no parent;
the numbers go into DESIGN.md 3.30.  Writes one JSON file.

    python scripts/bench_bodies.py [--lines 40] [--soundings 250] [--models 16] [--draws 64] [--few 8] [--columns 55 440] [--rounds 5]
                                   [--warmup 2] [--seed 0] [--out profiles/bodies/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_spatial_sections import ACROSS, events_ms, synthetic_survey      # noqa: E402
from geobipy_amd import _lib, bodies, sections      # noqa: E402
from geobipy_amd.ensembles import Ensemble      # noqa: E402

LO, HI, DEPTH = -1.0, float("inf"), 110.0                                     # the conductor: log10 S/m >= -1 in the top 110 m
TORCH_CHUNK_CELLS = 48 << 20                                                   # cells the torch statement labels at once


def torch_label(raster, eu, ev):
    """(label int32 [R, S, C], rounds): the rule stated in torch, as the module's docstring says."""
    R, S, C = raster.shape
    dev = raster.device
    N = S * C
    cell = torch.arange(N, device=dev).reshape(S, C)
    tu, tv = torch.as_tensor(eu).to(dev), torch.as_tensor(ev).to(dev)
    pi = torch.cat([cell[:, :-1].reshape(-1), cell[tu].reshape(-1)])
    pj = torch.cat([cell[:, 1:].reshape(-1), cell[tv].reshape(-1)])
    out = torch.empty((R, N), dtype=torch.int32, device=dev)
    chunk, rounds = max(1, TORCH_CHUNK_CELLS // N), 0
    for r0 in range(0, R, chunk):
        v = raster[r0:r0 + chunk].reshape(-1, N)
        n = v.shape[0]
        member = ((v >= LO) & (v <= HI)).reshape(-1)
        off = (torch.arange(n, device=dev) * N)[:, None]
        i, j = (pi[None, :] + off).reshape(-1), (pj[None, :] + off).reshape(-1)
        keep = member[i] & member[j]
        i, j = i[keep], j[keep]
        at = torch.arange(n * N, device=dev)
        lab = torch.where(member, at, torch.full_like(at, n * N))
        while True:
            before = lab.clone()
            lab.scatter_reduce_(0, i, lab[j], "amin")
            lab.scatter_reduce_(0, j, lab[i], "amin")
            lab = torch.where(member, torch.minimum(lab, lab[lab.clamp(max=n * N - 1)]), lab)
            rounds += 1
            if torch.equal(lab, before):                                      # the host waits here, once per round
                break
        out[r0:r0 + n] = torch.where(member, lab - off.expand(n, N).reshape(-1), torch.full_like(lab, -1)).reshape(n, N).to(torch.int32)
    return out.reshape(R, S, C), rounds


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--lines", type=int, default=40)
    p.add_argument("--soundings", type=int, default=250, help="per line")
    p.add_argument("--models", type=int, default=16)
    p.add_argument("--draws", type=int, default=64)
    p.add_argument("--few", type=int, default=8, help="a second, smaller number of realisations for the one-group case (0: skip)")
    p.add_argument("--columns", type=int, nargs="+", default=[55, 440])
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bodies", "bench.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_bodies needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.load()
    k, edges, sigma, x, y, ptr = synthetic_survey(a.lines, a.soundings, a.models, a.seed)
    S = k.shape[0]
    ens = Ensemble(torch.as_tensor(k).to(dev), torch.as_tensor(edges).to(dev), torch.as_tensor(sigma).to(dev), None, None, 1, None)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    slot = torch.randint(0, a.models, (a.draws, S), generator=gen, device=dev, dtype=torch.int32)
    graphs = {"lines": sections.line_edges(ptr) + (ptr,)}
    gu, gv, _, _ = sections.neighbours(x, y, ptr, None, max_distance=1.5 * ACROSS)
    graphs["graph"] = (gu.astype(np.int64), gv.astype(np.int64), np.array([0, S], dtype=np.int64))
    width = sections.section_widths(x, y, ptr)
    props = torch.cuda.get_device_properties(dev)
    result = dict(device=torch.cuda.get_device_name(dev), arch=getattr(props, "gcnArchName", ""), compute_units=props.multi_processor_count, lines=a.lines,
                  soundings_per_line=a.soundings, soundings=S, draws=a.draws, rounds=a.rounds, warmup=a.warmup, lo=LO, workgroup_threads=1024, cases=[])
    for C in a.columns:
        depth_edges = np.linspace(0.0, DEPTH, C + 1)
        whole = sections.draw_models(ens, slot, depth_edges=depth_edges)["raster"]
        t = np.diff(depth_edges)
        for name, (eu, ev, group_ptr) in graphs.items():
            for R in [a.draws] + ([a.few] if name == "graph" and 0 < a.few < a.draws else []):
                raster = whole[:R].contiguous()
                gp, gid = bodies.check_groups(group_ptr, eu, ev, S, "bench_bodies")
                order = np.argsort(gid, kind="stable")
                G, E = gp.size - 1, int(eu.size)
                t_eu, t_ev = (torch.as_tensor(v[order].astype(np.int32)).to(dev) for v in (eu, ev))
                t_gp, t_a, t_t = torch.as_tensor(gp).to(dev), torch.as_tensor(width).to(dev), torch.as_tensor(t).to(dev)
                unit = bodies.measure_unit(width, t)[2]
                label = torch.empty((R, S, C), dtype=torch.int32, device=dev)
                cells, mq = torch.empty_like(label), torch.empty((R, S, C), dtype=torch.int64, device=dev)
                sweeps = torch.empty((R, G), dtype=torch.int32, device=dev)

                def kernel():
                    _lib.call("gbp_bodies_label", dev, R, S, C, E, G, t_gp, t_eu, t_ev, raster, LO, HI, t_a, t_t, unit, label, cells, mq, sweeps)

                ms = {"kernel": [], "torch": []}
                rounds_torch = 0
                for r in range(a.warmup + a.rounds):
                    for which in ("kernel", "torch"):                         # taking turns
                        if which == "kernel":
                            took = events_ms(kernel, dev)
                        else:
                            box = []
                            took = events_ms(lambda: box.append(torch_label(raster, eu, ev)), dev)
                            stated, rounds_torch = box[0]
                        if r >= a.warmup:
                            ms[which].append(took)
                same = bool(torch.equal(stated, label))
                members = int((label >= 0).sum())
                case = dict(graph=name, columns=C, realisations=R, groups=G, workgroups=R * G, edges=E, cells=R * S * C, members=members,
                            bodies=int((cells > 0).sum()), largest_body_cells=int(cells.max()), sweeps_max=int(sweeps.max()), torch_rounds=rounds_torch,
                            ms_kernel=ms["kernel"], ms_torch=ms["torch"], seconds_kernel=float(np.median(ms["kernel"])) * 1e-3,
                            seconds_torch=float(np.median(ms["torch"])) * 1e-3, labels_equal=same)
                case["torch_over_kernel"] = case["seconds_torch"] / case["seconds_kernel"]
                result["cases"].append(case)
                print(json.dumps({n: case[n] for n in ("graph", "columns", "realisations", "workgroups", "sweeps_max", "torch_rounds", "seconds_kernel",
                                                       "seconds_torch", "torch_over_kernel", "labels_equal")}), flush=True)
                assert same, "the torch statement and the kernel disagree"
                del stated, label, cells, mq
        del whole
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
