#!/usr/bin/env python3
"""What graph propagation costs (HipEngine.graph_propagate, sml_amd.graph) at the Yelp shape: U = 60,000 users, I = 123,000 items,
a Seen of the Yelp history's size (five periods of 200,000 Zipf interactions, as tools/fold_in_probe.py builds it), fp32 and fp16
tables at d = 32 / 64 / 128.  It reports and does not judge.

  --series build      (no GPU) the library again with graph.hip compiled at every candidate split threshold, tools/_ab/
                      libsml_graph_s<S>.so for S in 1, 2, 4, 8, 16: the same C ABI, loaded beside the product's library
  --series measure    hops       one hop per side (users <- items over the set, items <- users over its transpose) and per (T, d) at
                                 path 0 / 1 / 2, with the member-row bytes gathered per second beside the 5.8 TB/s of bare random rows
                      threshold  the auto path of every candidate library on the same calls; the chosen value is the smallest S
                                 at which auto is not slower than either forced path beyond the run-to-run spread, at every pair
                      propagate  InteractionGraph.propagate(layers=3) end to end, per (T, d)
                      fit_step   one LightGCN step (forward, backward, Adam) at batch 8,192, fp32 d = 64
                      torch      the user-side hop in torch -- torch.sparse.mm on the normalised fp32 CSR, and index_select +
                                 index_add_ -- with time, peak extra memory and the largest difference from ours in units of the
                                 derived bound (40 + n_seg) 2^-23 |a| sum |b src|
  --series trace      the user-side call alone, 20 times (fp32, d = 64): run it under rocprofv3 --kernel-trace --stats

nine rounds that run every route once, in turn, after two warm-up rounds; medians, minima, interquartile spread.  Not measured:
trained tables, the recall of a fitted LightGCN on real periods, shapes beyond this one.  One JSON line on stdout (and --out).
usage: python tools/graph_probe.py --series build | measure [--out profiles/r24_graph_probe.json] | trace"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CANDIDATES = (1, 2, 4, 8, 16)
AB = os.path.join(HERE, "_ab")
SEG = 256
BARE_GATHER_TBS = 5.8
PAIRS = tuple((t, d) for d in (32, 64, 128) for t in ("fp32", "fp16"))


def note(msg):
    sys.stderr.write("[graph_probe] %s\n" % msg)
    sys.stderr.flush()


def variant_path(s):
    return os.path.join(AB, "libsml_graph_s%d.so" % s)


def build_variants():
    from sml_amd import build as B
    B.build()
    os.makedirs(AB, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = [os.path.join(B.CSRC, s.replace(".hip", ".o")) for s in B.SOURCES if s != "graph.hip"]
    for s in CANDIDATES:
        obj = os.path.join(AB, "graph_s%d.o" % s)
        subprocess.check_call([hipcc] + B.FLAGS + ["-DSML_GRAPH_SPLIT_FROM=%d" % s, "-c", os.path.join(B.CSRC, "graph.hip"), "-o", obj])
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", variant_path(s)] + objs + [obj])
        note("built %s" % variant_path(s))
    return 0


def yelp_sets(dev):
    from half_retrieval_probe import I, U
    from sml_amd import synth
    from sml_amd.retrieval import SeenItems
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        seen.add(train)
    return U, I, seen.device(dev), int(len(seen))


def tables(U, I, d, dtype, dev):
    gd = torch.Generator().manual_seed(d)
    t = torch.float32 if dtype == "fp32" else torch.float16
    return (torch.randn(U, d, generator=gd) * 0.3).to(dev).to(t), (torch.randn(I, d, generator=gd) * 0.3).to(dev).to(t)


def peak_extra_mb(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    del out
    return round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)


def gather_rate(pairs, d, elem_bytes, ms):
    tbs = pairs * d * elem_bytes / ms / 1e9
    return {"row_bytes": d * elem_bytes, "gathered_tb_per_s": round(tbs, 3), "of_bare_random_rows": round(tbs / BARE_GATHER_TBS, 3)}


def measure(args):
    from candidates_probe import rounds
    from half_retrieval_probe import stats, timed
    from sml_amd import _lib, graph
    from sml_amd.engine import HipEngine
    dev = torch.device("cuda:0")
    U, I, by_user, pairs = yelp_sets(dev)
    variants = {s: _lib.load_other(variant_path(s)) for s in CANDIDATES if os.path.exists(variant_path(s))}
    note("candidate libraries: %s" % sorted(variants))
    result = {"tool": "graph_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "seen_pairs": pairs, "reps": args.reps,
              "seg": SEG, "bare_random_rows_tb_per_s": BARE_GATHER_TBS, "hops": {}, "threshold": {"candidates": sorted(variants), "table": {}},
              "propagate_layers3": {}, "torch_user_hop": {},
              "not_measured": ["trained tables", "the recall of a fitted LightGCN on real periods", "shapes beyond the Yelp one"]}
    g = None
    for dtype, d in PAIRS:
        name = "d%d_%s" % (d, dtype)
        note(name)
        eng = HipEngine(dev, d, 256)
        if g is None:
            g = graph.InteractionGraph.build(by_user, U, I, engine=eng)
            lens_u, lens_i = (o[1:] - o[:-1] for o in (g.by_user[0], g.by_item[0]))
            result["split_from_built"] = eng.graph_split_from()
            result["rows_by_segments"] = {side: {"rows": int(l.shape[0]), "empty": int((l == 0).sum()), "one_segment": int(((l > 0) & (l <= SEG)).sum()),
                                                 "more": int((l > SEG).sum()), "max_members": int(l.max())}
                                          for side, l in (("users", lens_u), ("items", lens_i))}
        g._engine = eng
        wu, wi = tables(U, I, d, dtype, dev)
        eb = wu.element_size()
        sides = {"users": (wi, g.by_user, g.du, g.di), "items": (wu, g.by_item, g.di, g.du)}
        fns = {}
        for side, (src, sets, a, b) in sides.items():
            for path in (0, 1, 2):
                fns["%s_path%d" % (side, path)] = (lambda src=src, sets=sets, a=a, b=b, path=path:
                                                   eng.graph_propagate(src, sets, a=a, b=b, path=path))
            for s, lib in variants.items():
                e2 = HipEngine(dev, d, 256, lib=lib)
                fns["%s_auto_s%d" % (side, s)] = (lambda src=src, sets=sets, a=a, b=b, e2=e2: e2.graph_propagate(src, sets, a=a, b=b))
            fns["%s_path0_again" % side] = fns["%s_path0" % side]        # the same route at another place of the round: the A/A reading
        fns["propagate_layers3"] = lambda: g.propagate(wu, wi, layers=3)
        r = rounds(fns, args.reps, args.warmup, dev)
        for side, (src, sets, a, b) in sides.items():
            ref = eng.graph_propagate(src, sets, a=a, b=b, path=1)
            for key in [k for k in fns if k.startswith(side)]:
                r[key]["same_bytes_as_path1"] = bool(torch.equal(fns[key]().view(torch.int32), ref.view(torch.int32)))
                r[key].update(gather_rate(pairs, d, eb, r[key]["ms"]))
        result["hops"][name] = {k: v for k, v in r.items() if "_path" in k}
        result["threshold"]["table"][name] = {k: v for k, v in r.items() if "_auto_s" in k or "_path" in k}
        result["propagate_layers3"][name] = r["propagate_layers3"]
        if dtype == "fp32":
            result["torch_user_hop"][name] = torch_routes(eng, g, wi, lens_u, dev, args, stats, timed)
        if (dtype, d) == ("fp32", 64):
            result["fit_step_d64_fp32"] = fit_step(g, U, I, d, dev, args, stats, timed)
        del wu, wi, fns
        torch.cuda.empty_cache()
    result["threshold"].update(decide(result["threshold"]["table"], sorted(variants)))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


def decide(table, candidates):
    """The smallest S at which, for every (T, d) and side, auto's median is within the run-to-run spread of the faster forced
    path's.  The spread of a (pair, side) is the largest of the two readings' interquartile ranges and the A/A difference: the
    medians of the same route (path 0 of the built library) read at two places of the round."""
    verdict = {}
    for s in candidates:
        worst, ok = None, True
        for name, r in table.items():
            for side in ("users", "items"):
                auto = r["%s_auto_s%d" % (side, s)]
                forced = min((r["%s_path%d" % (side, p)] for p in (1, 2)), key=lambda x: x["ms"])
                aa = abs(r["%s_path0" % side]["ms"] - r["%s_path0_again" % side]["ms"])
                over = auto["ms"] - forced["ms"] - max(auto["iqr_ms"], forced["iqr_ms"], aa)
                if worst is None or over > worst[0]:
                    worst = (round(over, 4), name, side)
                ok = ok and over <= 0
        verdict[str(s)] = {"qualifies": ok, "worst_ms_beyond_spread": worst}
    chosen = next((s for s in candidates if verdict[str(s)]["qualifies"]), None)
    return {"verdict": verdict, "chosen": chosen, "note": None if chosen is not None else "no probed value qualifies"}


def torch_routes(eng, g, wi, lens_u, dev, args, stats, timed):
    off, items = g.by_user
    owner = torch.repeat_interleave(torch.arange(g.n_user, device=dev), lens_u)
    ours = eng.graph_propagate(wi, g.by_user, a=g.du, b=g.di)
    vals = g.du[owner] * g.di[items.long()]
    csr = torch.sparse_csr_tensor(off, items.long(), vals, size=(g.n_user, g.n_item))

    def by_index():
        rows = wi.index_select(0, items.long()) * g.di[items.long()].unsqueeze(1)
        return torch.zeros(g.n_user, wi.shape[1], device=dev).index_add_(0, owner, rows) * g.du.unsqueeze(1)

    mag = torch.zeros(g.n_user, wi.shape[1], device=dev, dtype=torch.float64).index_add_(
        0, owner, (wi.index_select(0, items.long()).double() * g.di[items.long()].double().unsqueeze(1)).abs()) * g.du.double().unsqueeze(1)
    bound = (40 + (lens_u + SEG - 1) // SEG).double().unsqueeze(1) * 2.0 ** -23 * mag
    out = {}
    for key, fn in (("sparse_mm", lambda: torch.sparse.mm(csr, wi)), ("index_select_index_add", by_index)):
        try:
            for _ in range(args.warmup):
                timed(fn, dev)
        except RuntimeError as e:            # a route this torch build does not have is reported, not hidden
            out[key] = {"error": str(e).splitlines()[0][:200]}
            continue
        ts = []
        for _ in range(args.reps):
            t, ref = timed(fn, dev)
            ts.append(t)
        diff = (ref.double() - ours.double()).abs()
        out[key] = dict(stats(ts), peak_extra_mb=peak_extra_mb(fn, dev),
                        largest_diff_in_units_of_the_bound=round(float((diff / bound.clamp(min=1e-300))[bound > 0].max()), 4))
        del ref
    out["csr_values_mb"] = round(vals.numel() * 4 / 2 ** 20, 1)
    return out


def fit_step(g, U, I, d, dev, args, stats, timed):
    from sml_amd.graph import LightGCN
    torch.manual_seed(0)
    model = LightGCN(U, I, d).to(dev).set_graph(g)
    opt = torch.optim.Adam([model.user_laten.weight, model.item_laten.weight], lr=1e-3)
    gen = torch.Generator(device=dev).manual_seed(0)
    off, items = g.by_user
    owner = torch.repeat_interleave(torch.arange(U, device=dev), off[1:] - off[:-1])
    idx = torch.randperm(owner.shape[0], device=dev, generator=gen)[:8192]
    u, i, n = owner[idx], items.long()[idx], torch.randint(0, I, (8192,), device=dev, generator=gen)

    def step():
        bpr, l2 = model(u, i, n)
        opt.zero_grad(set_to_none=True)
        (bpr + 1e-4 * l2).backward()
        opt.step()

    for _ in range(args.warmup):
        timed(step, dev)
    return dict(stats([timed(step, dev)[0] for _ in range(args.reps)]), batch=8192, layers=3)


def trace():
    from sml_amd import graph
    from sml_amd.engine import HipEngine
    dev = torch.device("cuda:0")
    U, I, by_user, _ = yelp_sets(dev)
    eng = HipEngine(dev, 64, 256)
    g = graph.InteractionGraph.build(by_user, U, I, engine=eng)
    _, wi = tables(U, I, 64, "fp32", dev)
    for _ in range(20):
        eng.graph_propagate(wi, g.by_user, a=g.du, b=g.di)
    torch.cuda.synchronize(dev)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", required=True, choices=("build", "measure", "trace"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.series == "build":
        return build_variants()
    return measure(args) if args.series == "measure" else trace()


if __name__ == "__main__":
    sys.exit(main())
