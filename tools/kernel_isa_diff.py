#!/usr/bin/env python3
"""Instruction streams of two hipcc -S listings, kernel by kernel: for kernels paired by meaning (RENAMED below, old name
-> new name; a kernel whose name is in both listings pairs with itself) the instruction counts and the lines that differ
once local labels are renumbered in order of appearance.  Shows whether a refactor of the entry points left the code alone.
Exit code 1 if a pair differs in length or a kernel of the first listing has no partner.
usage: python tools/kernel_isa_diff.py old.s new.s"""
import difflib
import re
import subprocess
import sys

# retrieval.hip: k_x / k_x_h / k_x_f / k_x_f_h <D> and k_x_a / k_x_a_h <D, F> became k_x<D, T, F, A>
RENAMED = {}
for fam in ("k_full_rank", "k_topk_slice", "k_ur_thresholds", "k_ur_count"):
    for suffix, t, widths in (("", "float", (32, 64)), ("_h", "half", (32, 64, 128))):
        for d in widths:
            RENAMED["%s%s<%d>" % (fam, suffix, d)] = "%s<%d, %s, false, false>" % (fam, d, t)
            RENAMED["%s_f%s<%d>" % (fam, suffix, d)] = "%s<%d, %s, true, false>" % (fam, d, t)
            for f in ("false", "true"):
                RENAMED["%s_a%s<%d, %s>" % (fam, suffix, d, f)] = "%s<%d, %s, %s, true>" % (fam, d, t, f)
for suffix, t, widths in (("", "float", (32, 64)), ("_h", "half", (32, 64, 128))):
    for d in widths:
        RENAMED["k_adjust_cosine%s<%d>" % (suffix, d)] = "k_adjust_cosine<%d, %s>" % (d, t)


def kernels(path):
    """demangled kernel name -> its instructions, comments dropped and local labels renumbered"""
    cur, data = None, {}
    for line in open(path):
        m = re.match(r"^(_Z\S+):\s", line)
        if m:
            cur = data.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            t = line.split(";")[0].strip()
            if t and (not t.startswith(".") or re.match(r"\.LBB\d+_\d+:", t)):      # instructions and local labels
                cur.append(t)
    text = "\n".join(n.replace("DF16_", "Dh") for n in data)
    names = subprocess.run(["c++filt"], input=text, capture_output=True, text=True).stdout.splitlines()
    out = {}
    for name, body in zip(names, data.values()):
        labels = {}
        body = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), t) for t in body]
        out[re.sub(r"\(anonymous namespace\)::|^void ", "", name).split("(")[0]] = body
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(old):
        partner = RENAMED.get(name, name)
        if partner not in new:
            print("%s -> %s: MISSING" % (name, partner))
            bad += 1
            continue
        a, b = old[name], new[partner]
        count = lambda body: sum(not t.endswith(":") for t in body)
        delta = [l for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[0] in "+-" and l[:3] not in ("+++", "---")]
        print("%s -> %s: %d / %d instructions, %d lines differ" % (name, partner, count(a), count(b), len(delta)))
        for l in delta:
            print("    " + l)
        bad += count(a) != count(b)
    print("pairs that differ in length or are missing:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
