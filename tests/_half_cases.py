"""Seeded fp16 cases for full-catalogue retrieval on half-precision tables: the GPU tests (test_half_retrieval_gpu.py) run
them, the host tests (test_half_retrieval_host.py) inspect them.  Tables are numpy float16; widen() is the exact fp32
copy the references of tests/_fp32_chain.py and tests/_user_rank_ref.py score."""
import numpy as np

import _fp32_chain as F


def widen(a):
    """float16 -> float32, exactly (every fp16 value is an fp32 value)."""
    return np.asarray(a, dtype=np.float16).astype(np.float32)


def random_half_case(d, seed=0, U=300, I=4099, n=256):
    """_fp32_chain.random_case with both tables rounded to fp16."""
    c = F.random_case(d, seed, U, I, n)
    c["wu"] = c["wu"].astype(np.float16)
    c["wi"] = c["wi"].astype(np.float16)
    return c


def dyadic_half(rng, rows, d):
    """entries k/8, |k| <= 16: every product and every sum over d <= 128 dims is exact in fp32 in any order."""
    return (rng.randint(-16, 17, size=(rows, d)) / 8.0).astype(np.float16)


def plant_specials(c, rng):
    """Subnormal halves, +-0, a NaN user row, a NaN item row and +-inf entries, in place.  Returns the NaN item."""
    wu, wi = c["wu"], c["wi"]
    for w in (wu, wi):
        m = rng.rand(*w.shape) < 0.05
        w[m] = (rng.randint(-1023, 1024, size=int(m.sum())) * 2.0 ** -24).astype(np.float16)     # subnormal halves (and 0)
        m = rng.rand(*w.shape) < 0.03
        w[m] = np.where(rng.rand(int(m.sum())) < 0.5, np.float16(0.0), np.float16(-0.0))
    assert ((np.abs(wi) < 2.0 ** -14) & (wi != 0)).sum() > 100 and np.signbit(wi[wi == 0]).any()
    wu[7] = np.nan
    wi[11] = np.nan
    wi[13, 3] = np.inf
    wi[17, 5] = -np.inf
    return 11


def half_near_tie_case(d, seed=0, ks=(1, 20, 128)):
    """_fp32_chain.near_tie_case in fp16: random fp16 tables with near-ties planted against the positives of rows 0..95
    and against the k-th entries of the lists:

    - exact copies of p's item row under other ids (ties: never counted, ordered by id in the lists);
    - copies with one coordinate moved to the next fp16 value up or down;
    - copies with dims permuted among coordinates where the user's row holds equal values, so the exact score is the
      positive's and only the rounding of the fp32 chain tells them apart (those users' rows hold every value twice);
    - copies of a user's k-th best item in other item slices.
    (Scores of fp16 tables are never fp32 subnormals -- the smallest product is 2^-48 -- so that family has no fp16 form;
    subnormal HALVES are in plant_specials.)"""
    c = random_half_case(d, seed)
    rng, wu, wi, rows, users = c["rng"], c["wu"], c["wi"], c["rows"], c["users"]
    I = wi.shape[0]
    planted = rows[:96]
    for u in np.unique(planted[:, 0]):
        half = rng.randn(d // 2).astype(np.float16)
        wu[u] = np.concatenate([half, half])[rng.permutation(d)]
    taken = set(rows[:, 1].tolist())
    free = [i for i in rng.permutation(I) if i not in taken]
    for u, p in planted:
        x = wi[p].copy()
        pairs = {}
        for q in range(d):
            pairs.setdefault(float(wu[u, q]), []).append(q)
        swaps = [g for g in pairs.values() if len(g) == 2]
        for _ in range(2):
            wi[free.pop()] = x
        for sgn in (1, -1):
            y = x.copy()
            q = rng.randint(d)
            y[q] = np.nextafter(y[q], np.float16(sgn * np.inf))
            wi[free.pop()] = y
        for _ in range(4):
            y = x.copy()
            for a, b in swaps:
                if rng.rand() < 0.5:
                    y[a], y[b] = y[b], y[a]
            wi[free.pop()] = y
    pick = users[:48]
    for j, u in enumerate(pick):
        k = ks[j % len(ks)]
        it, _ = F.ref_topk(widen(wu), widen(wi), [u], k, c["seen"])
        kth = it[0, -1]
        if kth < 0:
            continue
        for q in range(3):
            wi[free.pop()] = wi[kth]
    c.update(planted=planted, pick=pick)
    return c
