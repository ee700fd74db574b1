#!/usr/bin/env python3
"""The unweighted neighbourhood calls (HipEngine.cooc_topk and knn_topk) of the in-tree libsml_hip.so against another build of the
library (e.g. the previous commit's, built by hand into tools/_ab/), at the Yelp shape of tools/knn_probe.py, in one process.
Every round runs tree, other and a second copy of other once each, in turn: the two copies of the same build give that build's
own run-to-run spread, which is what the tree's difference is read against.  The outputs are compared for byte equality.
usage: python tools/knn_ab.py <other.so> <copy_of_other.so> [--reps 15] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from candidates_probe import rounds                              # noqa: E402
from half_retrieval_probe import I, U                            # noqa: E402
from knn_probe import K_NBR, TOPK                                # noqa: E402
from retrieval_ab import load_other                              # noqa: E402
from sml_amd import als, synth                                   # noqa: E402
from sml_amd.engine import HipEngine                             # noqa: E402
from sml_amd.retrieval import SeenItems                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("other_copy")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert os.path.realpath(args.other) != os.path.realpath(args.other_copy), "the copy must be a file of its own to be loaded twice"
    dev = torch.device("cuda:0")
    engines = {"tree": HipEngine(dev, 32, 256), "other": HipEngine(dev, 32, 256, lib=load_other(os.path.abspath(args.other))),
               "other_copy": HipEngine(dev, 32, 256, lib=load_other(os.path.abspath(args.other_copy)))}
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        seen.add(train)
    by_user = tuple(t.contiguous() for t in seen.device(dev))
    by_item = als.transpose_sets(by_user, U, I, engines["tree"])
    norm = (by_item[0][1:] - by_item[0][:-1]).double().sqrt()
    table = engines["tree"].cooc_topk(by_item, by_user, K_NBR, norm=norm)
    t_items, t_sims = table[0].to(torch.int32).contiguous(), table[1]
    fns, outs = {}, {}
    for name, eng in engines.items():
        fns["cooc_topk_" + name] = lambda eng=eng: eng.cooc_topk(by_item, by_user, K_NBR, norm=norm)
        fns["knn_topk_" + name] = lambda eng=eng: eng.knn_topk(t_items, t_sims, I, by_user, TOPK, seen=by_user)
        outs[name] = (fns["cooc_topk_" + name](), fns["knn_topk_" + name]())
    same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for call_t, call_o in zip(outs["tree"], outs["other"]) for a, b in zip(call_t, call_o))
    r = rounds(fns, args.reps, args.warmup, dev)
    result = {"tool": "knn_ab", "device": torch.cuda.get_device_name(dev), "other": os.path.basename(args.other), "U": U, "I": I,
              "seen_pairs": int(len(seen)), "k_nbr": K_NBR, "topK": TOPK, "reps": args.reps, "same_bytes": bool(same), "ms": r}
    for call in ("cooc_topk", "knn_topk"):
        t, o, c = (r["%s_%s" % (call, n)]["ms"] for n in ("tree", "other", "other_copy"))
        result[call] = {"tree_minus_other_ms": round(t - o, 4), "other_copy_minus_other_ms": round(c - o, 4),
                        "other_iqr_ms": r[call + "_other"]["iqr_ms"],
                        "inside_the_other_builds_own_spread": bool(abs(t - o) <= max(abs(c - o), r[call + "_other"]["iqr_ms"]))}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
