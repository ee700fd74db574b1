#!/usr/bin/env python3
"""What the neighbourhood model costs (HipEngine.cooc_topk / knn_topk, sml_amd.knn) at the Yelp shape: U = 60,000 users, I = 123,000
items, a Seen of the Yelp history's size (five periods of 200,000 Zipf interactions, as tools/fold_in_probe.py builds it),
k_nbr = 64 neighbours per item and lists of topK = 20.  One run records

  build       ItemNeighbours.build per metric (transpose, norm tables and the co-occurrence call), and the co-occurrence call
              alone: all items, the rows on each path, the heaviest row alone
  limit       the rows the on-chip path admits, in buckets of their total list length, forced through each path in turn
              (path = 1 / 2, alternated): the dense path's median beside the on-chip path's minimum, bucket by bucket -- the
              reading the limit's rule in DESIGN.md asks for
  atomics     the dense path's global integer atomics per second on the rows it serves (one add and one exchange per entry)
  recommend   ItemNeighbours.recommend with exclude = the history, for all users and for the one-to-five-item users alone
  torch       the routes the two calls replace, with their peak extra memory: torch.sparse.mm(X^T chunk, X) -> dense ->
              normalise -> topk for the build (timed on a few chunks of 2,048 items, the first -- the most popular items --
              among them; no full pass is timed), and a chunked gather of neighbour rows -> scatter_add_ into a dense
              [chunk, n_item] -> mask -> topk for the list; how often the torch list's items agree with ours where its float
              sums do not tie
  recall      one reading of evaluation.recall_of_lists for ItemKNN beside als.fit on one synthetic period (reported, not judged)

nine rounds that run every route once, in turn, after two warm-up rounds; medians, minima, interquartile spread.  Not measured:
real periods, trained tables for from_model, anything beyond this shape; the `fine` baseline's recall (it needs a training run).
One JSON line on stdout (and --out).
usage: python tools/knn_probe.py [--reps 9] [--out profiles/r23_knn_probe.json]"""
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
from sml_amd import als, evaluation, knn, synth                  # noqa: E402
from sml_amd.engine import HipEngine                             # noqa: E402
from sml_amd.mf import MFbasemode                                # noqa: E402
from sml_amd.retrieval import SeenItems, held_out, nonempty_users  # noqa: E402

K_NBR, TOPK = 64, 20
ITEM_CHUNK = 2048        # torch build: items per sparse product ([2048, 123000] fp32 dense = 1 GB)
USER_CHUNK = 2048        # torch list: users per dense accumulator ([2048, 123000] fp32 = 1 GB)
GUIDE_ATOMIC_TBPS = 1.3  # MI355X_MICROARCH.md, "Global float atomics": the chip-wide rate of added bytes, coalesced float adds


def note(msg):
    sys.stderr.write("[knn_probe] %s\n" % msg)
    sys.stderr.flush()


def torch_build_chunk(xt, x, deg_sqrt, c0, c1, k):
    """Cosine neighbours of items [c0, c1): one sparse product, made dense, normalised, the diagonal masked, topk."""
    rows = torch.arange(c0, c1, device=x.device)
    c = torch.sparse.mm(xt.index_select(0, rows), x).to_dense()
    s = c / (deg_sqrt[c0:c1].unsqueeze(1) * deg_sqrt.unsqueeze(0))
    s = torch.where(c > 0, s, s.new_full((), float("-inf")))
    s[torch.arange(c1 - c0, device=x.device), rows] = float("-inf")
    return torch.topk(s, k, dim=1)


def torch_list(nbr_items, nbr_sims, off, items, users, n_item, k):
    """The list of each user's history by a dense accumulator per chunk: gather, scatter_add_, mask the history, topk."""
    out_i, out_s = [], []
    for c0 in range(0, users.shape[0], USER_CHUNK):
        us = users[c0:c0 + USER_CHUNK]
        lens = off[us + 1] - off[us]
        owner = torch.repeat_interleave(torch.arange(us.shape[0], device=us.device), lens)
        start = torch.cumsum(lens, 0) - lens
        at = torch.repeat_interleave(off[us] - start, lens) + torch.arange(owner.shape[0], device=us.device)
        hist = items[at].long()
        ids, sims = nbr_items[hist], nbr_sims[hist]
        live = ids >= 0
        flat = (owner.unsqueeze(1) * n_item + ids.clamp(min=0)).reshape(-1)
        acc = torch.zeros(us.shape[0] * n_item, device=us.device, dtype=torch.float32)
        acc.scatter_add_(0, flat, torch.where(live, sims, sims.new_zeros(())).reshape(-1))
        touched = torch.zeros(us.shape[0] * n_item, device=us.device, dtype=torch.bool)
        touched[flat[live.reshape(-1)]] = True
        touched[owner * n_item + hist] = False                   # exclude = the history
        acc = torch.where(touched, acc, acc.new_full((), float("-inf"))).view(us.shape[0], n_item)
        s, i = torch.topk(acc, k, dim=1)
        out_i.append(torch.where(torch.isinf(s), i.new_full((), -1), i))
        out_s.append(s)
    return torch.cat(out_i), torch.cat(out_s)


def agreement(ours, theirs_i, theirs_s):
    """Of the slots whose torch score is separated from both neighbours by more than 1e-5 relative: how many hold our item."""
    s = theirs_s.double()
    gap = 1e-5 * s.abs().clamp(min=1e-30)
    pad = s.new_full((s.shape[0], 1), float("inf"))
    left = torch.cat([pad, s[:, :-1]], 1) - s
    right = s - torch.cat([s[:, 1:], -pad], 1)
    clear = torch.isfinite(s) & (left > gap) & (right > gap)
    # a tie or a near-tie moves only the slots inside its own group: a clear slot holds the same item on both routes
    clear[:, -1] = False                                          # (the last slot's right neighbour is not in the list)
    return int(clear.sum()), int((clear & (ours == theirs_i)).sum())


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
    users_of = by_item[1].long()
    owner_item = torch.repeat_interleave(torch.arange(I, device=dev), deg)
    total = torch.zeros(I, device=dev, dtype=torch.int64).index_add_(0, owner_item, lens_u[users_of])      # a row's total list length
    result = {"tool": "knn_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "seen_pairs": int(len(seen)),
              "k_nbr": K_NBR, "topK": TOPK, "lds_limit": limit, "reps": args.reps, "torch_reps": args.torch_reps,
              "users_by_items": {"0": int((lens_u == 0).sum()), "1..5": int(((lens_u > 0) & (lens_u <= 5)).sum()),
                                 ">5": int((lens_u > 5).sum()), "max": int(lens_u.max())},
              "cooc_rows": {"empty": int((total == 0).sum()), "on_chip": int(((total > 0) & (total <= limit)).sum()),
                            "dense": int((total > limit).sum()), "max_total": int(total.max()),
                            "entries_on_chip": int(total[total <= limit].sum()), "entries_dense": int(total[total > limit].sum())},
              "not_measured": ["real periods", "trained tables for from_model", "anything beyond the Yelp shape",
                               "the fine baseline's recall (it needs a training run)", "a full pass of the torch build route"]}
    note("rows: %s" % result["cooc_rows"])
    norm = deg.double().sqrt()
    rows_lds = torch.nonzero((total > 0) & (total <= limit)).reshape(-1)
    rows_dense = torch.nonzero(total > limit).reshape(-1)
    heaviest = torch.argmax(total).reshape(1)

    # ---- build -----------------------------------------------------------------------------------------------------------------
    fns = {"build_" + m: (lambda m=m: knn.ItemNeighbours.build(by_user, U, I, k=K_NBR, metric=m, engine=eng))
           for m in ("cosine", "asymmetric", "count")}
    fns.update({"cooc_all_rows": lambda: eng.cooc_topk(by_item, by_user, K_NBR, norm=norm),
                "cooc_on_chip_rows": lambda: eng.cooc_topk(by_item, by_user, K_NBR, rows=rows_lds, norm=norm),
                "cooc_dense_rows": lambda: eng.cooc_topk(by_item, by_user, K_NBR, rows=rows_dense, norm=norm),
                "cooc_heaviest_row": lambda: eng.cooc_topk(by_item, by_user, K_NBR, rows=heaviest, norm=norm)})
    note("build")
    result["build"] = rounds(fns, args.reps, args.warmup, dev)
    result["build"]["cooc_heaviest_row"]["total_list_length"] = int(total[heaviest])
    dense_ms = result["build"]["cooc_dense_rows"]["ms"]
    atomics = 2 * int(total[rows_dense].sum())                    # pass 1: one add per entry; pass 2: one exchange per entry
    result["atomics"] = {"dense_rows": int(rows_dense.shape[0]), "atomics": atomics, "giga_atomics_per_s": round(atomics / dense_ms / 1e6, 3),
                         "gb_per_s_of_4_byte_operands": round(4 * atomics / dense_ms / 1e6, 2),
                         "guide_chip_wide_float_add_gb_per_s": GUIDE_ATOMIC_TBPS * 1000,
                         "note": "scattered 4-byte integer atomics, one lane per address; the guide's figure is for coalesced float adds"}

    # ---- the limit's rule ------------------------------------------------------------------------------------------------------
    note("limit")
    result["limit"] = {}
    lo = 0
    for hi in (64, 128, 256, limit):
        rows = torch.nonzero((total > lo) & (total <= hi)).reshape(-1)
        lo = hi
        if rows.shape[0] == 0:
            continue
        td, tl, od, ol = alternate(lambda: eng.cooc_topk(by_item, by_user, K_NBR, rows=rows, norm=norm, path=1),
                                   lambda: eng.cooc_topk(by_item, by_user, K_NBR, rows=rows, norm=norm, path=2), args.reps, args.warmup, dev)
        result["limit"]["total<=%d" % hi] = {"rows": int(rows.shape[0]), "dense": stats(td), "on_chip": stats(tl),
                                            "same_bytes": bool(all(torch.equal(a, b) for a, b in zip(od, ol))),
                                            "dense_median_below_on_chip_min": bool(stats(td)["ms"] < stats(tl)["min_ms"])}

    # ---- recommend -------------------------------------------------------------------------------------------------------------
    note("recommend")
    nb = knn.ItemNeighbours.build(by_user, U, I, k=K_NBR, metric="cosine", engine=eng)
    all_users = torch.arange(U, device=dev)
    light = torch.nonzero((lens_u > 0) & (lens_u <= 5)).reshape(-1)
    fns = {"recommend_all_users": lambda: nb.recommend(by_user, topK=TOPK, exclude=by_user),
           "recommend_light_users": lambda: nb.recommend(by_user, users=light, topK=TOPK, exclude=by_user),
           "recommend_all_users_dense_path": lambda: eng.knn_topk(nb._narrow, nb.sims, I, by_user, TOPK, seen=by_user, path=1),
           "recommend_light_users_dense_path": lambda: eng.knn_topk(nb._narrow, nb.sims, I, by_user, TOPK, users=light, seen=by_user, path=1)}
    result["recommend"] = rounds(fns, args.reps, args.warmup, dev)
    result["recommend"]["light_users"] = int(light.shape[0])
    result["recommend"]["users_on_chip"] = int((lens_u * K_NBR <= limit).sum())

    # ---- the torch routes ------------------------------------------------------------------------------------------------------
    note("torch list")
    try:
        tl_fn = lambda: torch_list(nb._narrow.long(), nb.sims, by_user[0], by_user[1], all_users, I, TOPK)
        timed(tl_fn, dev)
        ts = []
        for _ in range(args.torch_reps):
            t, ref = timed(tl_fn, dev)
            ts.append(t)
        ours = nb.recommend(by_user, topK=TOPK, exclude=by_user)[0]
        clear, agree = agreement(ours, ref[0], ref[1])
        result["torch_list"] = dict(stats(ts), peak_extra_mb=peak_extra_mb(tl_fn, dev), user_chunk=USER_CHUNK, untied_slots=clear,
                                    untied_slots_with_our_item=agree)
        del ref
    except Exception as e:                                        # noqa: BLE001
        result["torch_list"] = {"error": repr(e)[:300]}
    torch.cuda.empty_cache()
    note("torch build")
    try:
        owner_user = torch.repeat_interleave(torch.arange(U, device=dev), lens_u)
        x = torch.sparse_coo_tensor(torch.stack([owner_user, by_user[1].long()]), torch.ones(owner_user.shape[0], device=dev),
                                    (U, I)).coalesce()
        xt = x.t().coalesce()
        chunks = [0, 1, 15, 30, 59]
        per = {}
        for c in chunks:
            c0, c1 = c * ITEM_CHUNK, min((c + 1) * ITEM_CHUNK, I)
            fn = lambda: torch_build_chunk(xt, x, norm.float(), c0, c1, K_NBR)
            timed(fn, dev)
            ts = [timed(fn, dev)[0] for _ in range(args.torch_reps)]
            ours = lambda: eng.cooc_topk(by_item, by_user, K_NBR, rows=torch.arange(c0, c1, device=dev), norm=norm)
            timed(ours, dev)
            to = [timed(ours, dev)[0] for _ in range(args.torch_reps)]
            per["items_%d..%d" % (c0, c1)] = {"torch": stats(ts), "cooc_topk_same_rows": stats(to),
                                              "torch_peak_extra_mb": peak_extra_mb(fn, dev)}
        result["torch_build_chunks"] = dict(per, item_chunk=ITEM_CHUNK, chunks_in_a_full_pass=(I + ITEM_CHUNK - 1) // ITEM_CHUNK)
        del x, xt
    except Exception as e:                                        # noqa: BLE001
        result["torch_build_chunks"] = {"error": repr(e)[:300]}
    torch.cuda.empty_cache()

    # ---- recall, one synthetic period: reported, not judged ----------------------------------------------------------------------
    note("recall")
    held = held_out(periods[5], U, I)
    users = nonempty_users(held)[0]
    ks = (5, 10, 20)
    lists = nb.recommend(by_user, users=users, topK=max(ks), exclude=by_user)[0]
    result["recall_one_synthetic_period"] = {"ks": list(ks), "users": int(len(users)),
                                             "itemknn_cosine": evaluation.recall_of_lists(lists, users, held, ks)}
    torch.manual_seed(0)
    model = MFbasemode(U, I, 32).to(dev)
    als.fit(model, by_user, sweeps=4, engine=eng)
    result["recall_one_synthetic_period"]["als_fit_d32_4_sweeps"] = evaluation.recall_curve(model, held, ks, exclude=seen)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
