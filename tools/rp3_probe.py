#!/usr/bin/env python3
"""What the weighted neighbours cost (HipEngine.cooc_topk_weighted, the rp3beta / p3alpha metrics of sml_amd.knn) at the Yelp shape
of tools/knn_probe.py: U = 60,000 users, I = 123,000 items, the same Seen (five periods of 200,000 Zipf interactions), k = 64
neighbours per item.  One run records

  build       ItemNeighbours.build for rp3beta and p3alpha beside the cosine and count builds, and the co-occurrence call alone,
              weighted (rp3beta's tables) beside unweighted (cosine's): all items, the rows the on-chip path admits, the rows of
              the dense path -- every route once per round, in turn, so the ratios are those of one run
  limit       the admitted rows, in buckets of their total list length, forced through each path in turn (path = 1 / 2,
              alternated), weighted call: the dense path's median beside the on-chip path's minimum, as r23 read it
  atomics     the dense path's global 8-byte integer atomics per second on the rows it serves
  torch       the route the call replaces, with its peak extra memory: torch.sparse.mm(X^T chunk, diag(w) X) -> dense -> divide
              by deg^alpha (x) deg^beta -> topk, timed on a few chunks of 2,048 items (no full pass is timed), and how often its
              items agree with ours on the slots where its float sums do not tie
  period      one synthetic period, reported and not judged: recall@5/10/20 and evaluation.popularity_of_lists of the lists of
              cosine against rp3beta at beta = 0 / 0.3 / 0.6

Not measured: real periods, trained comparisons, shapes beyond the Yelp one, sums above 2^53, a full pass of the torch route.
One JSON line on stdout (and --out).
usage: python tools/rp3_probe.py [--reps 9] [--out profiles/r25_rp3_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from candidates_probe import rounds                              # noqa: E402
from fold_in_probe import peak_extra_mb                          # noqa: E402
from half_retrieval_probe import I, U, alternate, stats, timed   # noqa: E402
from knn_probe import ITEM_CHUNK, K_NBR, agreement               # noqa: E402
from sml_amd import als, evaluation, knn, synth                  # noqa: E402
from sml_amd.engine import HipEngine                             # noqa: E402
from sml_amd.retrieval import SeenItems, held_out, nonempty_users  # noqa: E402

ALPHA, BETA = 1.0, 0.6


def note(msg):
    sys.stderr.write("[rp3_probe] %s\n" % msg)
    sys.stderr.flush()


def torch_build_chunk(xt, wx, na, nb, c0, c1, k):
    """RP3beta neighbours of items [c0, c1): one sparse product against the weighted matrix, made dense, divided, topk."""
    rows = torch.arange(c0, c1, device=wx.device)
    c = torch.sparse.mm(xt.index_select(0, rows), wx).to_dense()
    s = c / (na[c0:c1].unsqueeze(1) * nb.unsqueeze(0))
    s = torch.where(c > 0, s, s.new_full((), float("-inf")))
    s[torch.arange(c1 - c0, device=wx.device), rows] = float("-inf")
    return torch.topk(s, k, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch_reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = HipEngine(dev, 32, 256)
    limit = eng.knn_lds_limit()
    seen = SeenItems(U, I)
    periods = []
    for p in range(6):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        periods.append(train)
        if p < 5:
            seen.add(train)
    by_user = tuple(t.contiguous() for t in seen.device(dev))
    by_item = als.transpose_sets(by_user, U, I, eng)
    lens_u = by_user[0][1:] - by_user[0][:-1]
    deg = by_item[0][1:] - by_item[0][:-1]
    owner_item = torch.repeat_interleave(torch.arange(I, device=dev), deg)
    total = torch.zeros(I, device=dev, dtype=torch.int64).index_add_(0, owner_item, lens_u[by_item[1].long()])
    result = {"tool": "rp3_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "seen_pairs": int(len(seen)), "k_nbr": K_NBR,
              "alpha": ALPHA, "beta": BETA, "lds_limit": limit, "reps": args.reps, "torch_reps": args.torch_reps,
              "cooc_rows": {"empty": int((total == 0).sum()), "on_chip": int(((total > 0) & (total <= limit)).sum()),
                            "dense": int((total > limit).sum()), "entries_on_chip": int(total[total <= limit].sum()),
                            "entries_dense": int(total[total > limit].sum())},
              "not_measured": ["real periods", "trained comparisons", "shapes beyond the Yelp one", "sums above 2^53",
                               "a full pass of the torch route"]}
    note("rows: %s" % result["cooc_rows"])
    cos = deg.double().sqrt()
    rp3 = (deg.double().pow(ALPHA).contiguous(), deg.double().pow(BETA).contiguous())
    w = torch.where(lens_u > 0, lens_u.double().clamp(min=1.0).pow(-ALPHA), torch.zeros(U, device=dev, dtype=torch.float64)).float().contiguous()
    F = knn.frac_bits_for(float(w.max()))
    result["frac_bits"] = F
    rows_lds = torch.nonzero((total > 0) & (total <= limit)).reshape(-1)
    rows_dense = torch.nonzero(total > limit).reshape(-1)

    # ---- build -----------------------------------------------------------------------------------------------------------------
    fns = {"build_" + m: (lambda m=m: knn.ItemNeighbours.build(by_user, U, I, k=K_NBR, metric=m, engine=eng))
           for m in ("cosine", "count", "rp3beta", "p3alpha")}
    for name, rows in (("all_rows", None), ("on_chip_rows", rows_lds), ("dense_rows", rows_dense)):
        fns["cooc_" + name] = lambda rows=rows: eng.cooc_topk(by_item, by_user, K_NBR, rows=rows, norm=cos)
        fns["weighted_" + name] = lambda rows=rows: eng.cooc_topk_weighted(by_item, by_user, K_NBR, w, frac_bits=F, rows=rows, norm=rp3)
    fns["weighted_on_chip_rows_forced_dense"] = lambda: eng.cooc_topk_weighted(by_item, by_user, K_NBR, w, frac_bits=F, rows=rows_lds,
                                                                              norm=rp3, path=1)
    fns["cooc_on_chip_rows_forced_dense"] = lambda: eng.cooc_topk(by_item, by_user, K_NBR, rows=rows_lds, norm=cos, path=1)
    note("build")
    b = result["build"] = rounds(fns, args.reps, args.warmup, dev)
    result["weighted_over_unweighted"] = {
        "build_rp3beta_over_build_cosine": round(b["build_rp3beta"]["ms"] / b["build_cosine"]["ms"], 3),
        "build_p3alpha_over_build_cosine": round(b["build_p3alpha"]["ms"] / b["build_cosine"]["ms"], 3),
        "call_all_rows": round(b["weighted_all_rows"]["ms"] / b["cooc_all_rows"]["ms"], 3),
        "call_on_chip_rows": round(b["weighted_on_chip_rows"]["ms"] / b["cooc_on_chip_rows"]["ms"], 3),
        "call_dense_rows": round(b["weighted_dense_rows"]["ms"] / b["cooc_dense_rows"]["ms"], 3),
        "call_on_chip_rows_forced_dense": round(b["weighted_on_chip_rows_forced_dense"]["ms"] / b["cooc_on_chip_rows_forced_dense"]["ms"], 3)}
    atomics = 2 * int(total[rows_dense].sum())                    # pass 1: one add per entry; pass 2: one exchange per entry
    result["atomics"] = {"dense_rows": int(rows_dense.shape[0]), "atomics": atomics,
                         "giga_atomics_per_s_weighted": round(atomics / b["weighted_dense_rows"]["ms"] / 1e6, 3),
                         "giga_atomics_per_s_unweighted": round(atomics / b["cooc_dense_rows"]["ms"] / 1e6, 3),
                         "note": "scattered integer atomics, one lane per address: 8-byte operands weighted, 4-byte unweighted"}

    # ---- the limit's rule, weighted call -----------------------------------------------------------------------------------------
    note("limit")
    result["limit"] = {}
    lo = 0
    for hi in (64, 128, 256, limit):
        rows = torch.nonzero((total > lo) & (total <= hi)).reshape(-1)
        lo = hi
        if rows.shape[0] == 0:
            continue
        td, tl, od, ol = alternate(lambda: eng.cooc_topk_weighted(by_item, by_user, K_NBR, w, frac_bits=F, rows=rows, norm=rp3, path=1),
                                   lambda: eng.cooc_topk_weighted(by_item, by_user, K_NBR, w, frac_bits=F, rows=rows, norm=rp3, path=2),
                                   args.reps, args.warmup, dev)
        result["limit"]["total<=%d" % hi] = {"rows": int(rows.shape[0]), "dense": stats(td), "on_chip": stats(tl),
                                            "same_bytes": bool(all(torch.equal(a, b) for a, b in zip(od, ol))),
                                            "dense_median_below_on_chip_min": bool(stats(td)["ms"] < stats(tl)["min_ms"])}

    # ---- the torch route -------------------------------------------------------------------------------------------------------
    note("torch build")
    try:
        owner_user = torch.repeat_interleave(torch.arange(U, device=dev), lens_u)
        idx = torch.stack([owner_user, by_user[1].long()])
        x = torch.sparse_coo_tensor(idx, torch.ones(owner_user.shape[0], device=dev), (U, I)).coalesce()
        wx = torch.sparse_coo_tensor(idx, w[owner_user], (U, I)).coalesce()
        xt = x.t().coalesce()
        na, nb = rp3[0].float(), rp3[1].float()
        per = {}
        clear = agree = 0
        for c in (0, 1, 15, 30, 59):
            c0, c1 = c * ITEM_CHUNK, min((c + 1) * ITEM_CHUNK, I)
            fn = lambda: torch_build_chunk(xt, wx, na, nb, c0, c1, K_NBR)
            timed(fn, dev)
            ts, ref = [], None
            for _ in range(args.torch_reps):
                t, ref = timed(fn, dev)
                ts.append(t)
            rows = torch.arange(c0, c1, device=dev)
            ours = lambda: eng.cooc_topk_weighted(by_item, by_user, K_NBR, w, frac_bits=F, rows=rows, norm=rp3)
            timed(ours, dev)
            to, got = [], None
            for _ in range(args.torch_reps):
                t, got = timed(ours, dev)
                to.append(t)
            cl, ag = agreement(got[0], ref[1], ref[0])
            clear, agree = clear + cl, agree + ag
            per["items_%d..%d" % (c0, c1)] = {"torch": stats(ts), "cooc_topk_weighted_same_rows": stats(to),
                                              "torch_peak_extra_mb": peak_extra_mb(fn, dev), "untied_slots": cl,
                                              "untied_slots_with_our_item": ag}
        result["torch_build_chunks"] = dict(per, item_chunk=ITEM_CHUNK, chunks_in_a_full_pass=(I + ITEM_CHUNK - 1) // ITEM_CHUNK,
                                            untied_slots=clear, untied_slots_with_our_item=agree)
        del x, wx, xt
    except Exception as e:                                        # noqa: BLE001
        result["torch_build_chunks"] = {"error": repr(e)[:300]}
    torch.cuda.empty_cache()

    # ---- one synthetic period: reported, not judged ----------------------------------------------------------------------------
    note("period")
    held = held_out(periods[5], U, I)
    users = nonempty_users(held)[0]
    ks = (5, 10, 20)
    period = {"ks": list(ks), "users": int(len(users))}
    for name, kw in (("cosine", dict(metric="cosine")), ("rp3beta_beta_0", dict(metric="rp3beta", beta=0.0)),
                     ("rp3beta_beta_0.3", dict(metric="rp3beta", beta=0.3)), ("rp3beta_beta_0.6", dict(metric="rp3beta", beta=0.6))):
        nb = knn.ItemNeighbours.build(by_user, U, I, k=K_NBR, engine=eng, **kw)
        lists = nb.recommend(by_user, users=users, topK=max(ks), exclude=by_user)[0]
        period[name] = dict(evaluation.popularity_of_lists(lists, deg), recall=evaluation.recall_of_lists(lists, users, held, ks),
                            frac_bits=nb.frac_bits)
    result["one_synthetic_period"] = period
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
